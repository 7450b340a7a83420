/* gmpnp.h — C ABI of libgmpnp.so: MI355X (gfx950) backend for the GMPNP time-stepping Newton solve.
 *
 * Drop-in boundary.  The reference has no native code and no FFI; the operator API of its
 * hot path is the FEniCS call
 *     solve(F == 0, u, bcs, solver_parameters={'nonlinear_solver':'newton','newton_solver':{...}})
 * at 3D/MPNP_CO2ER_pore.py:789-799 and 1D/MPNP_CO2ER_EDL.py:717,729,737, fed by the objects built at
 * 3D:329-332 (Mesh), 3D:368-382 (boundary markers / ds), 3D:404-409 (MixedElement([P1]*9)),
 * 3D:425-432 (u, u_n), 3D:460-467 (DirichletBC list), 3D:474-769 (forms), 3D:856 (u_n.assign(u)) and
 * their 1D counterparts (1D:231-234, 300-306, 320-326, 350-355, 383-595, 796).  Each entry point below
 * names the reference construct it replaces.  A reference-side binding is a ctypes stub
 * (INTEGRATION.md).
 *
 * Conventions: plain C types; caller-allocated contiguous fp64 / int32 / int64 host buffers; all
 * vertex-indexed data in mesh-FILE vertex order, dof = vertex * n_fields + field (fields = species in
 * mixed-space order, potential last); the library owns all device memory behind the opaque handle;
 * every function returns 0 or a negative gmpnp_status and never throws; one host thread per handle; a handle
 * owns its HIP streams (the main one and a side stream for work that is off the critical path of a Newton
 * iteration, ordered by events) and a few pinned host cache lines the kernels report progress into; calls
 * block until their result is on the host (gmpnp_assign_previous is stream-ordered: it returns at once, and
 * whatever reads u_n next is queued behind the copy).
 */
#ifndef GMPNP_H
#define GMPNP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMPNP_MAX_SPECIES 8
#define GMPNP_MAX_BILINEAR 4
#define GMPNP_MAX_QUAD 16
#define GMPNP_MAX_NEWTON_HISTORY 64

typedef enum {
  GMPNP_OK = 0,
  GMPNP_ERR_INVALID = -1,        /* bad argument / unsupported configuration */
  GMPNP_ERR_HIP = -2,            /* HIP runtime error (see gmpnp_last_error)   */
  GMPNP_ERR_NOT_CONVERGED = -3,  /* Newton hit maximum_iterations ([3P] error_on_nonconvergence) */
  GMPNP_ERR_LINEAR = -4,         /* Krylov breakdown / did not reach tolerance / singular block */
  GMPNP_ERR_NUMERIC = -5         /* NaN residual or 1 - sum_j a_j u_j <= 0 at a quadrature point */
} gmpnp_status;

/* Coefficient tables of one member of the GMPNP weak-form family (replaces the UFL forms
 * 3D:505-769 / 1D:383-595 and the Constants feeding them 3D:261-324,474-499 / 1D:178-208,371-375).
 *   -R_i(u) = rc0_i + sum_j rc1_ij u_j + sum_t rc2_it u_{bil_j[t]} u_{bil_k[t]}
 *   eps(u)  = eps0 + sum_j epsc_j u_j ;  charge term  sum_j qzb_j u_j  (qzb_j = q z_j bulk_j)        */
typedef struct {
  int32_t dim;        /* 1 (interval) or 3 (tetrahedron) */
  int32_t n_species;  /* 6 (1D) or 8 (3D); n_fields = n_species + 1 */
  int32_t n_bilinear;
  int32_t steric;     /* 1 = MPNP (u_i/(1-S) term), 0 = PNP */
  double inv_dt;      /* 1/del_t (3D:534) or 1/(del_t*L_D) (1D:458) */
  double q;
  double eps0;
  double z[GMPNP_MAX_SPECIES];
  double a[GMPNP_MAX_SPECIES];    /* scale_vol */
  double qzb[GMPNP_MAX_SPECIES];
  double epsc[GMPNP_MAX_SPECIES];
  double rc0[GMPNP_MAX_SPECIES];
  double rc1[GMPNP_MAX_SPECIES][GMPNP_MAX_SPECIES];
  double rc2[GMPNP_MAX_SPECIES][GMPNP_MAX_BILINEAR];
  int32_t bil_j[GMPNP_MAX_BILINEAR];
  int32_t bil_k[GMPNP_MAX_BILINEAR];
  double wall_flux[GMPNP_MAX_SPECIES];   /* J_X_wall on ds(2)            3D:474-481 */
  double exit_kappa[GMPNP_MAX_SPECIES];  /* kappa_X (u_X - 1) on ds(3)   3D:484-499 */
  double point_flux[GMPNP_MAX_SPECIES];  /* J_X at the OHP vertex        1D:371-375,553,738 */
} gmpnp_model_t;

/* Quadrature of the rational steric integrand: barycentric points (first dim+1 entries of each row
 * used) and weights summing to 1, for the residual (degree 3) and the Jacobian (degree 4) — replaces the
 * FFC/FIAT-generated rules ([3P]). */
typedef struct {
  int32_t nq_f, nq_j;
  double lam_f[GMPNP_MAX_QUAD][4];
  double w_f[GMPNP_MAX_QUAD];
  double lam_j[GMPNP_MAX_QUAD][4];
  double w_j[GMPNP_MAX_QUAD];
} gmpnp_quadrature_t;

/* Mesh + boundary facet sets — replaces Mesh(...) 3D:329-332 / 1D:231-234, the marked ds measure
 * 3D:368-382 and FunctionSpace(mesh, MixedElement([P1]*n)) 3D:404-408 / 1D:300-304. */
typedef struct {
  int32_t dim;
  int32_t n_vertices;
  int32_t n_cells;
  const double* coords;        /* [n_vertices][dim] */
  const int32_t* cells;        /* [n_cells][dim+1]  */
  const int32_t* perm;         /* [n_vertices] internal->file vertex order, or NULL (identity).
                                  Contiguous internal ranges become the coarse-space aggregates and
                                  the multi-GPU partitions, so pass a slab ordering (see
                                  gmpnp_amd.backend.slab_permutation). */
  int32_t n_wall_facets;
  const int32_t* wall_facets;  /* [n][3] vertex triples of the exterior facets in ds(2) */
  int32_t n_exit_facets;
  const int32_t* exit_facets;  /* [n][3] ds(3) */
  int32_t n_point_vertices;
  const int32_t* point_vertices; /* 1D: vertices that receive model.point_flux */
} gmpnp_mesh_t;

/* Linear solver for J dx = b (replaces PETSc KSP preonly + LU: 'mumps' 3D:792, default LU 1D:357-364). */
typedef enum {
  GMPNP_LINEAR_BICGSTAB_TWOLEVEL = 0, /* BiCGStab, right-preconditioned by node-block Jacobi + slab-aggregate coarse correction */
  GMPNP_LINEAR_BICGSTAB_JACOBI = 1,   /* BiCGStab, node-block Jacobi only ([3P] 'bicgstab' + 'jacobi') */
  GMPNP_LINEAR_BLOCK_TRIDIAGONAL = 2, /* direct block-tridiagonal LU (1D meshes only) */
  GMPNP_LINEAR_BAND_LU = 3            /* direct block-banded LU in slab order (3D meshes); also what a 3D Krylov solve
                                         that does not converge falls back to, MUMPS never failing in the reference */
} gmpnp_linear_kind;

/* newton_solver parameter dict of the reference (3D:789-798, 1D:357-364) + krylov_solver sub-dict. */
typedef struct {
  int32_t maximum_iterations;   /* 50 */
  double relative_tolerance;    /* 1e-4 */
  double absolute_tolerance;    /* 1e-4 */
  double relaxation_parameter;  /* 0.9 (3D), 1.0 (1D) */
  int32_t linear_solver;        /* gmpnp_linear_kind */
  double krylov_relative_tolerance; /* on ||b - A x|| / ||b||; 1e-10 ~ "exact-equivalent" */
  double krylov_absolute_tolerance;
  int32_t krylov_maximum_iterations;
  double step_fraction;         /* tau of the fraction-to-boundary step limiter (below); 0 = off (plain damped Newton, bit for bit),
                                   else in (0, 1); anything else is GMPNP_ERR_INVALID.  No reference counterpart */
} gmpnp_newton_options_t;

/* Fraction-to-boundary step limiter (step_fraction = tau != 0; no reference counterpart: DOLFIN's NewtonSolver has none).  The
 * steric quotient u_i / (1 - S), S = sum_j a_j u_j, needs S < 1; an undamped correction can throw the iterate across S = 1, from
 * where Newton does not return (1 um mesh, Cs+, voltage_multiplier -10: the first solve diverges; a backtracking line search on
 * ||b|| stalls instead, because the residual has to rise first).  With dx the solution of J dx = b at the state u:
 *     S_I = sum_j a_j u_{I,j}     dS_I = sum_j a_j dx_{I,j}         (a = gmpnp_model_t.a, j ascending, plain fp64 sums)
 *     lambda = min over the VERTICES I with dS_I < 0 and S_I < 1 of (1 - S_I) / (-dS_I)      (+inf if there is none)
 *     alpha  = tau lambda if lambda < 1, else 1                     u <- u - relaxation_parameter alpha dx
 * S is P1, so admissible vertices give admissible quadrature points.  All rows take part, Dirichlet rows included; a vertex that
 * is inadmissible already (S_I >= 1) is skipped (no step length repairs it; steric_excursion reports it); model.steric = 0 (PNP)
 * evaluates the same rule with the model's a.  A NaN / Inf in dx ends the solve with GMPNP_ERR_NUMERIC and the update is not
 * applied.  Every linear solve of a limited Newton solve starts from zero: the predicted start of gmpnp_options_t.warm_start assumes
 * a constant step length.  Served by gmpnp_newton_solve (all linear solvers) and by 1D ensembles (per member: its own alpha,
 * statistics and failure); 3D ensembles and gmpnp_group_newton_solve refuse a non-zero step_fraction (GMPNP_ERR_INVALID). */

typedef struct {
  int32_t iterations;           /* Newton iterations performed ([3P] "Newton iteration k") */
  int32_t converged;
  int32_t krylov_iterations;    /* total over the solve */
  int32_t n_residuals;          /* iterations + 1 */
  double residuals[GMPNP_MAX_NEWTON_HISTORY]; /* ||b||_2 before iteration 0 and after each update */
  int32_t krylov_per_iteration[GMPNP_MAX_NEWTON_HISTORY];
  double ms_assemble, ms_setup, ms_krylov, ms_total; /* ms_total: host wall clock of the solve; the three phases are
                                                        device times (hipEvents), filled with gmpnp_options_t.phase_timing only */
  int32_t direct_solves;        /* Newton iterations whose system the block-banded LU solved (mode 3 or fallback) */
  int32_t steric_excursion;     /* 1 = some residual evaluation of this solve met 1 - sum_j a_j u_j <= 0 at a quadrature point
                                   (an iterate outside the admissible set).  UFL/FFC evaluate the quotient u_i/(1 - S) as it
                                   stands (3D:534-750, 1D:457-593), so by default this is information, not an error */
  int32_t limited_steps;        /* iterations whose update the step limiter shortened (alpha < 1); 0 with step_fraction = 0 */
  double min_step;              /* smallest alpha of the solve; 1.0 if never limited */
  double step_factor[GMPNP_MAX_NEWTON_HISTORY]; /* alpha of every iteration (step_fraction != 0; zeros otherwise) */
} gmpnp_newton_stats_t;

typedef struct {
  int32_t iterations;
  int32_t converged;
  double residual_norm;   /* recurrence ||r||_2 at exit */
  double rhs_norm;
} gmpnp_linear_stats_t;

/* Creation-time tunables (no reference counterpart). Zero-initialise for defaults: every field's 0 is the default. */
typedef struct {
  int32_t device_id;      /* HIP device ordinal */
  int32_t n_aggregates;   /* coarse-space slabs; 0 = default (8; at most 16 and what the LDS-resident coarse inverse allows) */
  int32_t shared_device;  /* 1 = other handles or processes use this GPU at the same time: no in-launch hand-over (four
                             launches per BiCGStab iteration) and no second HIP stream */
  int32_t krylov_batch;   /* iterations of the first burst of a BiCGStab solve; 0 = default (sized from the
                             previous solves; afterwards the host keeps one iteration queued ahead of the progress
                             the kernels report into pinned memory) */
  int32_t profile_every;  /* N > 0: the first burst of every Nth Krylov solve runs between a pair of HIP events (gmpnp_spmv_profile); 0 = off */
  int32_t launch_form;    /* launches per BiCGStab iteration: 0 = automatic (2 when hipOccupancyMaxActiveBlocksPerMultiprocessor
                             proves every workgroup of a launch resident at once, else 4), 2, 4.  Asking for 2 on a
                             problem that is not resident is refused (GMPNP_ERR_INVALID). */
  int32_t warm_start;     /* start of Newton iteration k+1's linear solve: 0 = second-order prediction from the two previous
                             corrections (default), 1 = first order, -1 = zero */
  int32_t coarse_refresh; /* coarse operator: 0 = rebuilt every Newton iteration on the side stream and adopted one iteration
                             later (default), N > 0 = rebuilt in the main stream every Nth Newton iteration */
  int32_t progress_by_copy; /* 1 = the host polls BiCGStab with a device-to-host copy + event per burst instead of the
                               pinned progress mirror */
  int32_t burst_iterations; /* iterations queued per poll after the first burst; 0 = 1 */
  int32_t phase_timing;   /* 1 = fill ms_assemble / ms_setup / ms_krylov of the Newton statistics (five event records
                             and one wait more per iteration) */
  int32_t no_direct_fallback; /* 1 = a 3D Krylov solve that does not converge is an error instead of a block-banded LU solve */
  int32_t warm_in_stream; /* 1 = the test of the predicted start runs in the main stream behind the set-up */
  int32_t vector_form;    /* BiCGStab half-iterations: 2 = the tile kernels recompute p / s at their column nodes on the fly (one launch
                             per half-iteration), 1 = streaming kernels write p / s for all rows first and the tile kernels stage
                             one vector (wins when the gathers cost memory bandwidth), 0 = automatic (1 above 768 MB of matrix) */
  int32_t strict_steric;  /* 1 = an iterate with 1 - sum_j a_j u_j <= 0 at a quadrature point ends the solve with GMPNP_ERR_NUMERIC
                             (rounds 1-2).  0 (default) = the reference's behaviour: no such test; an iterate that overshoots
                             and comes back converges, one that does not ends as NaN / not converged */
  int32_t element_stores; /* how the element kernel writes its per-cell records: 0 = automatic (3D: staged through LDS and written
                             record by record, up to 512 contiguous bytes per store instruction; 1D: direct), 1 = direct stores of
                             one lane per cell (every store instruction touches 64 records 1.6 KB apart), 2 = staged */
  double band_lu_max_gb;  /* largest band storage the direct solver may allocate; 0 = 48 */
} gmpnp_options_t;

typedef struct gmpnp_solver gmpnp_solver;

const char* gmpnp_version(void);
/* First 16 hex digits of the SHA-256 over the library's native sources (stamped by the build recipe, __graft_entry__.build):
 * measurements kept in the repository (PMC traffic per launch) name the build they were taken on. */
const char* gmpnp_build_id(void);
/* Message of the most recent failure on this thread. */
const char* gmpnp_last_error(void);

/* Mesh + FunctionSpace + forms -> device-resident problem. u and u_n start as zeros ([3P] Function(V), 3D:425). */
int gmpnp_create(const gmpnp_mesh_t* mesh, const gmpnp_model_t* model, const gmpnp_quadrature_t* quad,
                 const gmpnp_options_t* opts, gmpnp_solver** out);
void gmpnp_destroy(gmpnp_solver* s);

/* Re-upload constants (Constant(...) objects rebuilt between steps: del_t 1D:639-642 (Q2), J_OH/J_H 1D:789-793). */
int gmpnp_set_model(gmpnp_solver* s, const gmpnp_model_t* model);

/* SUPG stabilisation of the PNP model, reference 1D/MPNP_CO2ER_EDL.py:597-722 (--model PNP --stabilization Y; 1D
 * meshes only): F gets  - sum_i rho_i z_i [ (u_i - u_i^n)/(dt L_D) + z_i grad(w_i).grad(p) + R_i ] grad(p).grad(v_i) dx
 * with the P1 field rho_i given by its vertex values rho[vertex*n_species + i] (0 = species not stabilised; the
 * reference recomputes them every time step from the previous potential, 1D:650-685) and w_i = u_{w_index[i]} (NULL =
 * identity; the reference's OH term takes grad(u_H)). rho = NULL switches the terms off. */
int gmpnp_set_supg(gmpnp_solver* s, const double* rho, const int32_t* w_index);

/* bcs list after DOLFIN's in-order application (later wins): unique dofs + values (3D:460-467,835-838; 1D:350-355). */
int gmpnp_set_dirichlet(gmpnp_solver* s, int64_t n, const int64_t* dofs, const double* values);

/* u / u_n contents (either pointer may be NULL to leave that vector untouched). interpolate 3D:432, project 1D:326. */
int gmpnp_set_state(gmpnp_solver* s, const double* u, const double* u_n);
/* compute_vertex_values() of all fields at once (3D:802-813, 1D:745-753). */
int gmpnp_get_state(gmpnp_solver* s, double* u_out, double* u_n_out);
/* u_n.assign(u) (3D:856, 1D:796), on device. */
int gmpnp_assign_previous(gmpnp_solver* s);

/* ---- adaptive time stepping with error control (no reference counterpart: the reference marches with the step of its YAML file) ----
 * Backward Euler with a step chosen from an estimate of its local error; the accept / reject rule itself is host code
 * (csrc/gmpnp_host_rules.h, next_time_step; gmpnp_amd/timestep.py drives it).  The handle keeps a third state vector, u_nm1 = the
 * accepted state before u_n.  Over the FREE dofs (I, f) — a Dirichlet dof's change between steps is boundary data moving, not
 * truncation error — with h the step just solved and h_prev the accepted step before it (the units of 1 / inv_dt up to a factor
 * the caller owns: only h / h_prev and the rate's scale depend on them):
 *     p = u_n + (h / h_prev)(u_n - u_nm1)        d = (u - p) h / (2h + h_prev)        w = atol_f + rtol max(|u|, |u_n|)
 *     err_f = sqrt(sum_I (d/w)^2 / n_free_f)     rate_f = sqrt(sum_I ((u - u_n)/h)^2 / n_free_f)
 * (u - p = 1/2 u'' h (2h + h_prev) + O(h^3), so d is backward Euler's local error 1/2 u'' h^2.)  There is no history when no step
 * was accepted since create / a gmpnp_set_state that wrote u_n / gmpnp_assign_previous, or when h_prev <= 0: has_history = 0 and the err values are
 * 0; the rates are computed all the same.  A field without a free dof reports 0.  worst_dof: ties go to the smaller index of the
 * handle's internal order.  A NaN / Inf in u sets nonfinite and makes the err values NaN; the status stays GMPNP_OK (the caller
 * decides).  Fixed-order reductions, no atomics: two calls on one state return the same bits.  u_nm1 and the estimator's storage
 * are allocated by the first call of this family; a handle that never calls it keeps the buffers and launches it had.  Partition
 * handles (gmpnp_create_partition) are refused by all four calls (GMPNP_ERR_INVALID): groups have no adaptive stepping.  The
 * members of an ensemble step adaptively, each on its own clock, through the batched forms of these calls
 * (gmpnp_ensemble_set_time_step, gmpnp_ensemble_time_error, gmpnp_ensemble_time_advance below). */
typedef struct { double rtol; double atol[GMPNP_MAX_SPECIES + 1]; } gmpnp_time_tol_t;
typedef struct {
  double err;                                  /* max_f err_field[f]; 0 when there is no history */
  double err_field[GMPNP_MAX_SPECIES + 1];
  double rate;                                 /* max_f rate_field[f] */
  double rate_field[GMPNP_MAX_SPECIES + 1];
  int64_t worst_dof;                           /* file order (vertex*n_fields+field) of max |d/w|, -1: none */
  int32_t has_history, nonfinite;
} gmpnp_time_error_t;
/* model.inv_dt alone, on the host and the device, of this handle AND of every coarse level attached below it with
 * gmpnp_attach_coarse_level (gmpnp_set_model leaves those as they are; the time term is the diagonal of the species blocks, so a
 * stale coarse level costs Krylov iterations).  Invalidates the Jacobian and the preconditioner.  inv_dt finite and >= 0 (0 = the
 * steady form); NaN, Inf and negative values are GMPNP_ERR_INVALID.  The boundary tables are NOT rebuilt: checked against
 * rebuild_boundary (gmpnp_api.hip) — wall_flux, exit_kappa, point_flux and the facet areas are all it reads, and the SUPG
 * parameters (gmpnp_set_supg) are the caller's. */
int gmpnp_set_time_step(gmpnp_solver* s, double inv_dt);
int gmpnp_time_error(gmpnp_solver* s, double h, double h_prev, const gmpnp_time_tol_t* tol, gmpnp_time_error_t* out);
/* u_nm1 <- u_n, u_n <- u in one launch (stream-ordered like gmpnp_assign_previous, which it replaces in an adaptive run: calling
 * gmpnp_assign_previous afterwards drops the history, has_history = 0, because u_nm1 was not shifted with it). */
int gmpnp_time_accept(gmpnp_solver* s);
/* u <- u_n (device copy); the history stays.  The next Newton solve starts from a state set from outside (no coarse reuse). */
int gmpnp_time_reject(gmpnp_solver* s);

/* ---- second-order adaptive time stepping: variable-step BDF2 (opt-in; kernels: csrc/gmpnp_time_order.h) ----
 * A handle that never calls gmpnp_set_time_order(s, 2) keeps the buffers, launches and results of the calls above.  With
 * omega = h / h_prev the BDF2 time term is (alpha0 / h) M (u - u*), alpha0 = (1 + 2 omega)/(1 + omega),
 * u* = ((1 + omega)^2 u_n - omega^2 u_nm1)/(1 + 2 omega): the shape of backward Euler's inv_dt M (u - u_n) with another scalar and
 * another vector, so the residual, the Jacobian and the species budgets of an order-2 step come from the same kernels.  The handle
 * counts the accepted states behind u_n (levels: 0, 1 = u_nm1, 2 = u_nm1 and u_nm2); gmpnp_time_accept raises the count,
 * gmpnp_time_reject keeps it, a gmpnp_set_state that writes u_n and gmpnp_assign_previous reset it to 0.  has_history of the calls
 * above is levels >= 1.  The estimator of an order-2 step, over the free dofs, h1 / h2 the two accepted steps before h:
 *     p = the quadratic through (t - h1 - h2, u_nm2), (t - h1, u_nm1), (t, u_n) at t + h
 *     d = (u - p) kappa,  kappa = c / (h + h1 + h2 + c),  c = h / alpha0        w, err_f, rate_f, worst_dof, nonfinite: as above
 * (u_exact - p = u'''/6 h (h + h1)(h + h1 + h2) and BDF2's local error is u'''/6 h^2 (h + h1)(1 + omega)/(1 + 2 omega), the same sign:
 * kappa is the second's share of their sum.)  The coefficients are host functions of csrc/gmpnp_host_rules.h, where the
 * accept / reject rule of order 2 lives too (next_time_step with order = 2).  Partition handles are refused (GMPNP_ERR_INVALID), and
 * so is every gmpnp_ensemble_* call that solves, estimates or advances while a member is at order 2. */
/* order 1 (backward Euler, the default) or 2.  2 allocates u_nm2 and u* on the first call; from then on gmpnp_time_accept shifts
 * three deep (u_nm2 <- u_nm1 <- u_n <- u, one launch) and counts up to 2 levels.  1 makes the time term read u_n again and caps the
 * levels at 1. */
int gmpnp_set_time_order(gmpnp_solver* s, int32_t order);
int gmpnp_time_history_levels(gmpnp_solver* s, int32_t* levels);
/* The set-up of a BDF2 step: u* is formed on the device (one launch), model.inv_dt becomes alpha0(ratio) * inv_dt on the host and the
 * device of this handle and of every attached coarse level, the time term reads u* in u_n's place, the Jacobian and the
 * preconditioner are invalidated.  inv_dt as gmpnp_set_time_step's; ratio = h / h_prev finite and > 0; the handle at order 2 with
 * levels >= 1.  A later gmpnp_set_time_step is a backward Euler step again and reads u_n.  gmpnp_get_state, the estimators,
 * gmpnp_time_reject and the rate of change always see the true u_n. */
int gmpnp_set_time_step_bdf2(gmpnp_solver* s, double inv_dt, double ratio);
/* The estimator above for the step u_n -> u of length h (h_prev, h_prev2: the two accepted steps before it).  With fewer than 2
 * levels, or h_prev <= 0 or h_prev2 <= 0: has_history = 0 and the err values are 0, the rates are computed all the same.  Fixed-order
 * reductions: two calls give the same bits. */
int gmpnp_time_error_bdf2(gmpnp_solver* s, double h, double h_prev, double h_prev2, const gmpnp_time_tol_t* tol, gmpnp_time_error_t* out);
/* u* of the last gmpnp_set_time_step_bdf2, file order [n_dofs] (for tests). */
int gmpnp_get_time_history(gmpnp_solver* s, double* out);

/* solve(F == 0, u, bcs, solver_parameters) (3D:789-799, 1D:737-742): damped Newton on the device state u.
 * Returns GMPNP_ERR_NOT_CONVERGED where DOLFIN raises RuntimeError; stats are filled either way. */
int gmpnp_newton_solve(gmpnp_solver* s, const gmpnp_newton_options_t* opts, gmpnp_newton_stats_t* stats);

/* ---- lower-level hooks for parity tests and benchmarks ([3P] assemble / DirichletBC.apply / KSP) ---- */
/* The step limiter's rule (gmpnp_newton_options_t.step_fraction) evaluated on the device at the handle's current u for a
 * correction dx given in FILE order (n_dofs), with the kernels the Newton loop runs: *alpha, *lambda (+inf: no limiting vertex)
 * and *node = the limiting vertex in mesh-FILE numbering (-1 = none; equal ratios: the first in the handle's internal order).
 * tau in (0, 1).  Changes nothing: u, u_n, the Jacobian and the solver's vectors stay as they were.  A NaN / Inf in dx returns
 * GMPNP_ERR_NUMERIC.  Outputs may be NULL. */
int gmpnp_step_limit(gmpnp_solver* s, const double* dx, double tau, double* alpha, double* lambda, int64_t* node);
int32_t gmpnp_n_fields(const gmpnp_solver* s);
int64_t gmpnp_n_dofs(const gmpnp_solver* s);
int64_t gmpnp_n_blocks(const gmpnp_solver* s);   /* node blocks of the BSR Jacobian */
int64_t gmpnp_jacobian_nnz(const gmpnp_solver* s); /* n_blocks * n_fields^2 */
int32_t gmpnp_n_aggregates(const gmpnp_solver* s);
/* Kernel launches per BiCGStab iteration of the 3D solver: 4 (coarse, tile, coarse, tile) or 2 (the coarse workgroups
 * ride inside the tile launches; chosen when the occupancy query proves all workgroups of a launch resident at once; gmpnp_options_t.launch_form
 * overrides). Diagnostics for the bench; no reference counterpart. */
int32_t gmpnp_krylov_launches_per_iteration(const gmpnp_solver* s);

/* b = assemble(F) with bc rows b = x - g; optionally A = assemble(J) with identity bc rows (kept on device).
 * F_out (n_dofs) and norm_out may be NULL. */
int gmpnp_assemble(gmpnp_solver* s, int32_t want_jacobian, double* F_out, double* norm_out);
/* Current device Jacobian as CSR in file-order dof numbering, columns ascending (indptr n_dofs+1, others nnz). */
int gmpnp_get_jacobian_csr(gmpnp_solver* s, int32_t* indptr, int32_t* indices, double* data);
/* y = J x with the current device Jacobian. */
int gmpnp_spmv(gmpnp_solver* s, const double* x, double* y);
/* y = As x with the column-scaled Jacobian As = J blockdiag(J_II)^-1 of the last preconditioner set-up, read as the Krylov kernels read it (needs a set-up: a linear or Newton solve on this Jacobian). */
int gmpnp_spmv_scaled(gmpnp_solver* s, const double* x, double* y);
/* Solve J x = b with the current device Jacobian (preconditioner is rebuilt). */
int gmpnp_linear_solve(gmpnp_solver* s, const double* b, double* x, int32_t linear_solver, double rtol,
                       double atol, int32_t max_iterations, gmpnp_linear_stats_t* stats);

/* ---- post-processing on the device ------------------------------------------------------------
 * project(sign * grad(f), W).compute_vertex_values() of a P1 field f given by its vertex values (file order): the
 * consistent-mass L2 projection of the cell-wise constant gradient the reference computes for `field_values` and the
 * `<X>_grad` arrays (1D/MPNP_CO2ER_EDL.py:802-805, 3D/MPNP_CO2ER_pore.py:884-909).  out: [n_vertices][dim], row major.
 * Jacobi-preconditioned CG on the P1 mass matrix to 1e-14 relative residual; stats (may be NULL) reports the iterations. */
int gmpnp_project_gradient(gmpnp_solver* s, const double* nodal_values, double sign, double* out, gmpnp_linear_stats_t* stats);
/* project(f, Y) of a cell-wise constant field with ncomp <= 4 components, cell_values [n_cells][ncomp] in mesh-file cell order
 * (reference 1D:599 project(CellDiameter(mesh)), 1D:651-653 the projected gradient norm of the SUPG parameters). out: [n_vertices][ncomp]. */
int gmpnp_project_cellwise(gmpnp_solver* s, int32_t ncomp, const double* cell_values, double* out, gmpnp_linear_stats_t* stats);

/* ---- mesh-partitioned solve (no reference counterpart: the reference is a serial script) -------------
 * One handle per rank on the rank's LOCAL mesh = every cell that touches an owned vertex; the other vertices of those cells
 * are ghosts (owned by a neighbouring rank), flagged as Dirichlet dofs by the caller so that their matrix rows are identity
 * rows.  Cut cells are assembled on both sides, so owned rows are complete without matrix communication.  Inside the
 * library: ghost rows of (r, v, p) / (s, t) travel after each BiCGStab half-iteration (grouped ncclSend/ncclRecv on the
 * solver's stream), the dot products and the coarse restrictions of a half-iteration travel in ONE ncclAllReduce, the
 * coarse operator is GLOBAL (slabs numbered over the whole mesh, one all-reduce of the Galerkin matrix per set-up, inverted
 * redundantly by every rank).  gmpnp_amd/dist.py builds the partition and the plan. */
typedef struct {
  int32_t rank, size;
  int32_t n_global_aggregates;       /* coarse slabs over the WHOLE mesh (<= 15 for 9 fields) */
  const int32_t* vertex_aggregate;   /* [n_vertices] slab of each LOCAL vertex (local mesh-file order); mesh.perm must run
                                        through the slabs in ascending order */
  const uint8_t* vertex_owned;       /* [n_vertices] 1 = owned by this rank, 0 = ghost; a slab is all owned or all ghost */
  int32_t n_neighbours;
  const int32_t* neighbour_rank;     /* [n_neighbours] */
  const int32_t* send_ptr;           /* [n_neighbours+1] into send_vertices */
  const int32_t* send_vertices;      /* local vertices whose rows go to neighbour q, in q's receive order */
  const int32_t* recv_ptr;           /* [n_neighbours+1] into recv_vertices */
  const int32_t* recv_vertices;      /* local ghost vertices filled from neighbour q, in q's send order */
} gmpnp_partition_t;

int gmpnp_create_partition(const gmpnp_mesh_t* local_mesh, const gmpnp_model_t* model, const gmpnp_quadrature_t* quad,
                           const gmpnp_options_t* opts, const gmpnp_partition_t* part, gmpnp_solver** out);

/* RCCL communicator of the ranks (one process per GPU).  Rank 0 makes the id and hands the 128 bytes to the others by any
 * means (the Python driver broadcasts them with torch.distributed); every rank then joins.  librccl.so is loaded on first
 * use; its absence is an error here, not at library load. */
#define GMPNP_COMM_ID_BYTES 128
typedef struct gmpnp_comm gmpnp_comm;
int gmpnp_comm_unique_id(char id[GMPNP_COMM_ID_BYTES]);
int gmpnp_comm_create(const char id[GMPNP_COMM_ID_BYTES], int32_t rank, int32_t size, int32_t device_id, gmpnp_comm** out);
/* n doubles sent to this rank itself and received back (grouped ncclSend + ncclRecv), then all-reduced over the communicator:
 * exercises every RCCL entry point of the partitioned solve; max_error = largest deviation from the expected sums. */
int gmpnp_comm_selftest(gmpnp_comm* c, int32_t n, double* max_error);
void gmpnp_comm_destroy(gmpnp_comm* c);

/* The partition handles ONE PROCESS drives: exactly one with a communicator (production: one rank per GPU), or all `size`
 * of them with comm = NULL (rehearsal of the whole partitioned algorithm inside one process on one GPU: the exchanges
 * become device copies between the handles; this is what the single-GPU test box runs). */
typedef struct gmpnp_group gmpnp_group;
int gmpnp_group_create(int32_t n_local, gmpnp_solver* const* handles, gmpnp_comm* comm, gmpnp_group** out);
/* Third transport: the caller moves the bytes.  The library stages each all-reduce / ghost exchange through pinned host
 * buffers and calls back; the Python driver implements the two calls with torch.distributed on `gloo`.  For machines
 * without RCCL between the ranks and for the two-ranks-on-one-card test (RCCL refuses two ranks on one device); every
 * collective costs two PCIe copies and a stream synchronisation, so this is not a production path.
 *   allreduce(user, buf, n):  sum buf[0..n) over all ranks, in place, same result on every rank; 0 = ok
 *   exchange(user, n_neighbours, neighbour_rank, send_offset, send_count, send_buf, recv_offset, recv_count, recv_buf):
 *       send send_buf[send_offset[j] .. +send_count[j]) (doubles) to neighbour j, receive its message into
 *       recv_buf[recv_offset[j] .. +recv_count[j]); 0 = ok */
typedef struct {
  int32_t rank, size;
  int (*allreduce)(void* user, double* buf, int32_t n);
  int (*exchange)(void* user, int32_t n_neighbours, const int32_t* neighbour_rank, const int64_t* send_offset, const int64_t* send_count,
                  const double* send_buf, const int64_t* recv_offset, const int64_t* recv_count, double* recv_buf);
  void* user;
} gmpnp_host_transport_t;
int gmpnp_group_create_hosted(gmpnp_solver* handle, const gmpnp_host_transport_t* transport, gmpnp_group** out);
/* Fourth transport: peer mailboxes — the one to use with one process per GPU.  Every rank owns a mailbox in its GPU's memory
 * (uncached), mapped into the other ranks' processes through an IPC handle; a collective is ONE kernel launch per rank that
 * stores its contribution / its ghost rows straight into the other ranks' mailboxes (xGMI between GPUs), raises a flag there
 * and waits for the flags in its own: no collective library and no host step between two BiCGStab half-iterations.
 *   1. every rank: gmpnp_group_peer_begin(handle, &group, my_handle)         -> 64 bytes to publish
 *   2. the caller gathers the handles of all ranks in rank order (any channel; this gather is also the point after which
 *      every mailbox exists), then every rank: gmpnp_group_peer_connect(group, all_handles)
 *   3. gmpnp_group_newton_solve ... ; before gmpnp_group_destroy the caller makes sure (a barrier of its own) that no rank is
 *      still inside a solve.
 * A rank that does not arrive within 5 s ends the others' launch with an error instead of a hang. */
#define GMPNP_PEER_HANDLE_BYTES 64
int gmpnp_group_peer_begin(gmpnp_solver* handle, gmpnp_group** out, char ipc_handle[GMPNP_PEER_HANDLE_BYTES]);
int gmpnp_group_peer_connect(gmpnp_group* g, const char* all_handles);
void gmpnp_group_destroy(gmpnp_group* g);
/* solve(F == 0, u, bcs, solver_parameters) on the partitioned state (each handle's u / u_n hold owned + ghost values, set
 * with gmpnp_set_state; ghost values of u are kept current inside).  Collective: every rank calls it.  Statistics are
 * identical on all ranks.  Linear solver: GMPNP_LINEAR_BICGSTAB_TWOLEVEL or _JACOBI. */
int gmpnp_group_newton_solve(gmpnp_group* g, const gmpnp_newton_options_t* opts, gmpnp_newton_stats_t* stats);
/* u_n.assign(u) on every local handle. */
/* One pass of each collective of the partitioned solve over the group's own transport with self-checking contents (an all-reduce
 * of 5 doubles, one ghost-row message per neighbour; on a peer-mailbox group that will run its solves with the exchange inside the
 * next launch, the same contents once more through the flagged-word areas those launches use): *max_error = largest deviation this
 * process saw (0 expected).  Collective:
 * every rank calls it.  No reference counterpart (the reference is serial); it is the start-up check of BASELINE configs[3]. */
int gmpnp_group_selftest(gmpnp_group* g, double* max_error);
/* Peer-mailbox groups: how the exchange of a BiCGStab half-iteration's sums and boundary rows is launched.  form 0 (default) = in
 * front of the NEXT half-iteration's coarse workgroups, inside that launch (two launches per iteration, as on one GPU), wherever
 * the launch with its exchange workgroups is resident at once; form 1 = its own launch between the two (four per iteration).
 * Every rank of a partition must run the same form: the caller compares gmpnp_group_exchange_form over the ranks after set-up and
 * sets form 1 everywhere unless all of them report 2 (gmpnp_amd/dist.py does).  gmpnp_group_exchange_form: what a solve
 * of this group will do — 2 = exchange inside the next launch, 1 = separate launches, 0 = not a peer-mailbox group.  No reference
 * counterpart. */
int gmpnp_group_set_exchange_form(gmpnp_group* g, int32_t form);
int32_t gmpnp_group_exchange_form(const gmpnp_group* g);
int gmpnp_group_assign_previous(gmpnp_group* g);

/* Geometric multilevel term of the preconditioner on uniformly refined meshes (no reference counterpart: the reference solves
 * with MUMPS, 3D:792; this keeps the iteration count of the Krylov stand-in from growing with the refinement level).
 * `coarse` is an ordinary handle of the PARENT mesh of `fine`'s mesh (same model; its Dirichlet set decides its identity rows);
 * parents[2 v + {0, 1}] = the two coarse vertices (coarse FILE order) fine vertex v (fine file order) interpolates from, both the
 * same vertex when v is a copy of it (red refinement: every fine vertex is one or the other).  From then on every preconditioner
 * set-up of `fine` injects the state into `coarse`, assembles the Jacobian there and sets up the coarse handle's own two-level
 * preconditioner M_c^-1, and M^-1 of `fine` gains  theta * P S_c P^T  (additive), S_c = `sweeps` Richardson sweeps x <- x +
 * PRE_c (r - J_c x) from x = 0 with PRE_c = M_c^-1 + [the same term for a level attached below `coarse`] — sweeps = 1 is purely
 * additive, every further sweep costs one SpMV with J_c (1/8 of a fine one) (csrc/gmpnp_multilevel.h).
 * Chains: attach level 2 to level 1, then level 1 to level 0.  `coarse` must outlive `fine` and must not be driven by the caller
 * any more.  BiCGStab then runs in the materialised vector form.  3D handles on one device.
 * Partition handles (gmpnp_create_partition): `fine` and `coarse` are handles of the SAME rank of partitions of the same size, the
 * coarse plan derived from the fine one (gmpnp_amd/dist.py partition_hierarchy: a coarse vertex is owned where its copy is, and both
 * parents of every owned fine vertex are local); parents are in the two handles' LOCAL file orders, -1 where a parent is not local
 * (ghost rows only).  The levels of all ranks then form groups of their own, attached with gmpnp_group_attach_coarse_group. */
int gmpnp_attach_coarse_level(gmpnp_solver* fine, gmpnp_solver* coarse, const int32_t* parents, double theta, int32_t sweeps);
/* Multilevel term of a mesh-partitioned solve: `coarse` is a group (gmpnp_group_create / _create_hosted, the same communicator for
 * RCCL) of the coarse-level handles attached to `fine`'s handles, rank by rank, over the same transport kind; it carries that level's
 * halo exchanges and all-reduces from now on (chains: attach level 2's group to level 1's, level 1's to level 0's).
 * gmpnp_group_newton_solve of `fine` then runs the V-cycle across the partitioned levels in every BiCGStab half-iteration (two-level
 * mode only); `coarse` must outlive `fine` and is not driven by itself any more.  Refused (GMPNP_ERR_INVALID): peer-mailbox groups,
 * groups of another transport kind or rank count, handles that are not the attached levels.  No reference counterpart. */
int gmpnp_group_attach_coarse_group(gmpnp_group* fine, gmpnp_group* coarse);

/* ---- order statistics of the state's vertex columns on the device -----------------------------------------------------------
 * Replaces the per-step host glue of the reference's time loop, 3D/MPNP_CO2ER_pore.py:817-838: np.median of the H / OH / HCO3 /
 * cation vertex arrays (the Sechenov update of the CO2 Dirichlet value) and the minimum of the CO2 array.  k-th smallest values of
 * owned vertex columns of u (global over the group's ranks for the group form).  ncols selections: field[j] in [0, n_fields),
 * rank[j] in [0, n_global_vertices) (n <= 64).  Returns in out[j] the value NumPy's np.sort(column)[rank[j]] holds (-0.0 counts as
 * +0.0; subnormals and +-Inf are ordinary values).  *flags bit 0 = a selected column holds a NaN (out[] undefined for it).
 * Exact radix select on the 64-bit keys of the doubles (csrc/gmpnp_stats.h): eight histogram passes, the integer counts all-reduced
 * over the group's transport, one host synchronisation per call; the result is the same bit for bit on every transport and rank
 * count.  The group form is collective (every rank calls it with the same selections); rank[j] not below the global number of
 * owned rows is GMPNP_ERR_INVALID on every rank. */
int gmpnp_column_select(gmpnp_solver* s, int32_t n, const int32_t* field, const int64_t* rank, double* out, int32_t* flags);
int gmpnp_group_column_select(gmpnp_group* g, int32_t n, const int32_t* field, const int64_t* rank, double* out, int32_t* flags);

/* ---- species budgets and consistent boundary fluxes on the device (no reference counterpart: the reference writes fields only) ----
 * P1 test functions sum to one, so the RAW residual rows of one field (before Dirichlet rows are overwritten) sum to that field's
 * integrated balance; terms whose test-function factor is a gradient (diffusion, migration, steric, SUPG) drop out of the sum.  Per
 * field f (species 0 .. n_species-1 in model order, potential last) one row of GMPNP_BUDGET_COLUMNS doubles in the scaled units of the
 * weak form, evaluated at the current u / u_n / model / Dirichlet set:
 *   inventory  int u_f dx                                   storage  inv_dt int (u_f - u_f^n) dx   (0 for the potential)
 *   reaction   int (rc0 + sum rc1 u + sum rc2 u u) dx = int -R_f;  potential row: the space-charge term sum_j qzb_j int u_j dx
 *   wall       wall_flux_f |S2|        exit  exit_kappa_f int_S3 (u_f - 1) ds        point  point_flux_f x number of point vertices
 *   dirichlet  sum of the raw residual over the Dirichlet dofs of f: the consistent flux the constraint supplies
 *   closure    sum of the raw residual over the free dofs of f: bounded by sqrt(n_free) times the Newton residual
 * with  storage + reaction + wall + exit + point = dirichlet + closure  to rounding for any state (the left side from closed-form
 * P1 integrals, the right side from the gathered element rows: independent arithmetic).  Fixed-order reductions: two calls on one
 * state return the same bits.  The call evaluates the element residual itself, into storage of its own: u, u_n, F, the Jacobian,
 * the preconditioner and every policy state of the handle stay as they were.  Sums run over the handle's OWNED rows; the group form
 * adds the ranks' tables with the group's all-reduce (collective: every rank calls it; the same table on every rank). */
#define GMPNP_BUDGET_COLUMNS 8
typedef enum {
  GMPNP_BUDGET_INVENTORY = 0,
  GMPNP_BUDGET_STORAGE = 1,
  GMPNP_BUDGET_REACTION = 2,
  GMPNP_BUDGET_WALL = 3,
  GMPNP_BUDGET_EXIT = 4,
  GMPNP_BUDGET_POINT = 5,
  GMPNP_BUDGET_DIRICHLET = 6,
  GMPNP_BUDGET_CLOSURE = 7
} gmpnp_budget_column;
int gmpnp_species_budget(gmpnp_solver* s, double* out /* [n_fields][GMPNP_BUDGET_COLUMNS] */);
int gmpnp_group_species_budget(gmpnp_group* g, double* out /* [n_fields][GMPNP_BUDGET_COLUMNS] */);

/* ---- Stern-layer boundary condition (no reference counterpart: the reference prescribes the potential at the outer Helmholtz plane
 * and 1D/Stern_CO2ER.py integrates the Stern layer afterwards) -----------------------------------------------------------------------
 * On the Stern boundary Gamma_S (1D: the point vertices, the OHP vertex; 3D: the wall facets ds(2)) the potential row keeps the
 * boundary term of its integration by parts, with displacement continuity across an ion-free layer of scaled thickness lam:
 *     F_p += int_{Gamma_S} g(eps) (p_M - p) / lam  v ds        eps = eps0 + sum_j epsc_j u_j
 * p_electrode = p_M in thermal voltages; model 1 (linear): g = eps; model 2 (BDM): g = (eps - eps_s) / ln(eps / eps_s) with
 * eps_s = eps_surface (ignored by model 1).  1D takes eps at the vertex; 3D takes it per facet at the facet mean of u and (p_M - p) as
 * P1 with the facet mass matrix |f| (1 + delta_ab) / 12.  The Jacobian holds the exact derivative, the permittivity's included.  A
 * potential row that carries a Dirichlet value receives nothing (the caller leaves the OHP potential out of gmpnp_set_dirichlet).
 * eps <= 0 on Gamma_S under model 2 raises status bit 32: the residual evaluation (gmpnp_assemble, gmpnp_newton_solve) returns
 * GMPNP_ERR_NUMERIC.  gmpnp_species_budget reports the integrated term in the potential row's wall (3D) or point (1D) column.
 * Setting the option invalidates the Jacobian and the preconditioner; model = 0 restores the handle as it was before the first call
 * (no launch, no buffer read).  Refused (GMPNP_ERR_INVALID, the message names Stern): partition handles (and so groups), a handle with
 * a coarse level attached or serving as one (and attaching one to a handle with the option on), every gmpnp_ensemble_* call with such a
 * member.  gmpnp_stern_displacement: the integrated term int_{Gamma_S} g (p_M - p) / lam ds at the current u, scaled units. */
typedef struct {
  int32_t model;       /* 0 off, 1 linear, 2 BDM */
  double p_electrode;  /* p_M [thermal voltages] */
  double lam;          /* Stern length / length scale of the mesh, > 0 */
  double eps_surface;  /* eps_s of the BDM model, > 0 */
} gmpnp_stern_t;
int gmpnp_set_stern(gmpnp_solver* s, const gmpnp_stern_t* stern);
int gmpnp_stern_displacement(gmpnp_solver* s, double* out);

/* ---- potential-dependent surface kinetics (no reference counterpart: the reference prescribes the current through the constant
 * wall_flux / point_flux) ---------------------------------------------------------------------------------------------------------
 * Up to GMPNP_MAX_SURFACE_REACTIONS reactions on the Stern boundary Gamma_S (the node set of gmpnp_set_stern: 1D the point vertices,
 * 3D the vertices of the wall facets).  Reaction r has a rate constant k, a transfer coefficient alpha, an equilibrium offset p_eq
 * (thermal voltages), an optional first-order reactant (species index, -1 = none) and flux weights nu[r][i] per species.  With
 * p_M = p_electrode, at boundary node I:
 *     E_r    = exp(-alpha_r (p_M - p_I - p_eq_r))            rate_r = k_r (reactant_r >= 0 ? u_{I,reactant_r} : 1) E_r
 *     F[(I,i)]                += w_I sum_r nu[r][i] rate_r                  (species rows i only)
 *     J[(I,i),(I,reactant_r)] += w_I nu[r][i] k_r E_r          J[(I,i),(I,p)] += w_I nu[r][i] alpha_r rate_r
 * w_I = 1 in 1D; in 3D the sum over the wall facets holding I of |f| / 3 in facet list order (vertex quadrature, the weight the
 * constant wall_flux enters with).  The sign is that of point_flux / wall_flux: one reaction with reactant -1, alpha 0, k 1 and
 * nu = J is the constant flux J.  The reactant is not clamped.  A species row that carries a Dirichlet value receives nothing.  A
 * rate that is not finite raises status bit 64: the residual evaluation (gmpnp_assemble, gmpnp_newton_solve) returns
 * GMPNP_ERR_NUMERIC.  gmpnp_species_budget adds the integrated kinetic flux of species i to its wall (3D) / point (1D) column.
 * Setting the option invalidates the Jacobian and the preconditioner; n_reactions = 0 on a handle that never had the option changes
 * nothing, and after the option has been on it restores F and J bit for bit.  Independent of gmpnp_set_stern (a Dirichlet potential
 * on Gamma_S makes E_r a constant); the two work together.  Refused (GMPNP_ERR_INVALID, the message names kinetics): partition
 * handles (and so groups), a handle with a coarse level attached or serving as one (and attaching one to a handle with the option
 * on), every gmpnp_ensemble_* call with such a member, a handle with SUPG terms set (and gmpnp_set_supg with the option on), a mesh
 * without a Stern boundary.  gmpnp_kinetics_currents: out[r] = sum_I w_I rate_r at the current u. */
#define GMPNP_MAX_SURFACE_REACTIONS 4
typedef struct {
  int32_t n_reactions;                                   /* 0 = off */
  int32_t reactant[GMPNP_MAX_SURFACE_REACTIONS];         /* species index, -1 = none */
  double k[GMPNP_MAX_SURFACE_REACTIONS];
  double alpha[GMPNP_MAX_SURFACE_REACTIONS];
  double p_eq[GMPNP_MAX_SURFACE_REACTIONS];              /* thermal voltages */
  double nu[GMPNP_MAX_SURFACE_REACTIONS][GMPNP_MAX_SPECIES];
  double p_electrode;                                    /* p_M [thermal voltages] */
} gmpnp_kinetics_t;
int gmpnp_set_kinetics(gmpnp_solver* s, const gmpnp_kinetics_t* kinetics);
int gmpnp_kinetics_currents(gmpnp_solver* s, double* out /* [n_reactions] */);

/* ---- galvanostatic mode (no reference counterpart: the reference prescribes the current through constant fluxes; with the surface
 * kinetics the current follows the potential, and this option solves the inverse problem) ------------------------------------------
 * The electrode potential p_M becomes one extra scalar unknown of the handle and one extra equation fixes the total kinetic current.
 * With I_r(u, p_M) = sum_I w_I rate_r (gmpnp_kinetics_currents) and I = sum_r weight[r] I_r:
 *     G(u, p_M) = ln(I / target) = 0                                     target > 0, I > 0
 *     c = dG/du   at boundary node I: column reactant_r: weight_r w_I k_r E_r / I,  column p: weight_r w_I alpha_r rate_r / I
 *     d = dG/dp_M = -sum_r weight_r alpha_r I_r / I
 *     b = dF/dp_M  Stern rows: 1D g / lam, 3D sum over the node's Stern facets in list order of g(eps_f) |f| / (3 lam);
 *                  kinetic rows: -w_I sum_r nu[r][i] alpha_r rate_r;  0 on every Dirichlet row and everywhere else
 * gmpnp_newton_solve then runs a bordered Newton iteration by block elimination:
 *     J y = F,  J z = b,  dp = (G - c.y) / (d - c.z),  dx = y - dp z,  u -= omega alpha dx,  p_M -= omega alpha dp
 * (alpha: the step limiter's factor, 1 without it; the limiter looks at u only).  The residual the convergence test sees is
 * sqrt(||F||^2 + G^2), before the first iteration and after every update.  I <= 0, a value of I, G, c.y, c.z or dp that is not finite
 * or d - c.z == 0 raise status bit 128: the update is not applied and the solve ends GMPNP_ERR_NUMERIC.  The logarithm makes the
 * Tafel law linear in p_M; the difference form (I - target) / target leaves the admissible set from ordinary starts.
 * 1D handles take GMPNP_LINEAR_BLOCK_TRIDIAGONAL (two solves per iteration), 3D handles GMPNP_LINEAR_BAND_LU (one factorisation, two
 * substitutions); the BiCGStab solvers are refused with the option on.
 * gmpnp_set_galvanostat needs the kinetics on, a finite target > 0 and finite weights that are not all zero.  p_M starts at the
 * kinetics' p_electrode; with the Stern option on, its p_electrode must be equal to it.  on = 0 on a handle that never had the option
 * is a no-op; after the option has been on it writes the current p_M into both options' p_electrode, and from then on F and J are
 * bit for bit those of a handle that had that p_electrode set directly.  While the option is on gmpnp_set_kinetics and
 * gmpnp_set_stern keep the galvanostat's p_M (their p_electrode is not read) and n_reactions = 0 is refused.  gmpnp_assign_previous
 * and gmpnp_time_accept copy p_M to its twin at u_n, gmpnp_time_reject copies it back.  gmpnp_species_budget,
 * gmpnp_kinetics_currents and gmpnp_stern_displacement see the current p_M.  Refused (GMPNP_ERR_INVALID, the message names the
 * galvanostat): partition handles (and so groups), a handle with a coarse level attached or serving as one, every gmpnp_ensemble_*
 * call with such a member, order-2 time stepping.
 * gmpnp_galvanostat_report: p_M now and at u_n, the currents and G at the current u, and c.y, c.z, d, dp, alpha of the last
 * iteration of the last solve (zeros before one).  gmpnp_galvanostat_terms: parity hook; at the current u and p_M, b in file order
 * (b_out[n_dofs], may be NULL) and scalars[4] = {G, d, I, c.x} for the caller's x (file order; NULL: c.x = 0). */
typedef struct {
  int32_t on;                                    /* 0 = off */
  double target;                                 /* I_target > 0, in the units of sum_I w_I rate_r */
  double weight[GMPNP_MAX_SURFACE_REACTIONS];    /* weight_r of reaction r in the total current */
} gmpnp_galvanostat_t;
typedef struct {
  double p_electrode, p_electrode_n;             /* p_M now and at u_n */
  double I_r[GMPNP_MAX_SURFACE_REACTIONS];       /* sum_I w_I rate_r at the current u */
  double I, G;
  double cy, cz, d, dp, alpha;                   /* the last iteration's c.y, c.z, d, dp and step factor */
} gmpnp_galvanostat_report_t;
int gmpnp_set_galvanostat(gmpnp_solver* s, const gmpnp_galvanostat_t* galvanostat);
int gmpnp_galvanostat_report(gmpnp_solver* s, gmpnp_galvanostat_report_t* out);
int gmpnp_galvanostat_terms(gmpnp_solver* s, const double* x /* [n_dofs] or NULL */, double* b_out /* [n_dofs] or NULL */, double* scalars /* [4] */);

/* ---- small-signal frequency response (no reference counterpart: impedance spectroscopy of the double layer) ------------------------
 * 1D handles with the Stern option on.  The linearisation is taken at the handle's current u and p_M: K = J(u) at inv_dt = 0 with
 * every Stern and kinetic term and the Dirichlet identity rows, M = the consistent P1 mass on the species rows that carry no Dirichlet
 * value (J is affine in inv_dt: J = K + inv_dt M), b = dF/dp_M as the galvanostatic mode defines it.  Per unit of p_M (thermal
 * voltages), at time-term multiplier sigma >= 0 with i sigma in the place of inv_dt:
 *     (K + i sigma M) x = -b
 *     C(sigma)    = dD/dp_M + (dD/du).x        D = gmpnp_stern_displacement; 1D: dD/dp_M = g / lam, dD/dp_v = -g / lam, dD/du_{v,j} =
 *                                              g' epsc_j (p_M - p_v) / lam (the Stern row of J)
 *     dI_r(sigma) = dI_r/dp_M + (dI_r/du).x    I_r = gmpnp_kinetics_currents; = -alpha_r I_r + sum_I w_I (k_r E_r x_reactant + alpha_r rate_r x_p)
 * Nothing depends on u_n or on model.inv_dt.  out[k] holds sigma[k], C and dI_r as (re, im) pairs (dI = 0 with the kinetics off), the
 * residual max |(K + i sigma M) x + b| / max |b| and a status word of that frequency alone: bit 256 = a pivot of the complex block
 * elimination was (all but) zero, bit 512 = a value that is not finite; the other frequencies are not affected.  x_out, where given,
 * receives x as (re, im) pairs in file order.  The n systems are solved by a complex block Thomas elimination with partial pivoting
 * inside the 7 x 7 blocks (pivot key |re| + |im|), eight lanes per frequency, in chunks of frequencies sized from a memory cap
 * (1024 MB of workspace; the environment variable GMPNP_RESPONSE_CAP_MB overrides it) with one host synchronisation per chunk; the
 * result of a frequency does not depend on n or on the chunking, and two calls give equal bits.  Afterwards F, the Jacobian and the
 * validity flags of the handle are what they were before the call, bit for bit (a following gmpnp_newton_solve is not affected).
 * Refused (GMPNP_ERR_INVALID, the message names the frequency response): 3D handles, partition handles, SUPG terms set, a coarse
 * level attached or serving as one, the Stern option off, the galvanostat on (switch it off first: that keeps the potential it
 * found), Stern and kinetic options with different p_electrode, n outside 1 ... 4096, a sigma that is negative or not finite.
 * eps <= 0 on the Stern boundary or a rate that is not finite at the current state: GMPNP_ERR_NUMERIC. */
typedef struct {
  double sigma;
  double C[2];                                   /* (re, im), scaled units */
  double dI[GMPNP_MAX_SURFACE_REACTIONS][2];     /* (re, im) per reaction */
  double residual;
  int32_t status;                                /* 0, or bits 256 / 512 */
} gmpnp_response_t;
int gmpnp_frequency_response(gmpnp_solver* s, int32_t n, const double* sigma /* [n] */, gmpnp_response_t* out /* [n] */,
                             double* x_out /* [n][n_dofs][2] in file order, or NULL */);

/* ---- frequency response, 3D (the same response on the 3D pore: a complex block-banded LU) ------------------------------------------
 * 3D handles with the Stern option on; arguments, records and semantics of gmpnp_frequency_response with the 3D terms of the
 * galvanostat and of the tangent: K = J(u) at inv_dt = 0 with the Stern rows facet by facet, the kinetic rows and the Dirichlet
 * identity rows; M = the consistent P1 tetrahedron mass (vol / 20 (1 + delta_ab), formed from the mesh as the Jacobian gather forms it,
 * one double per node block) on the species rows that carry no Dirichlet value; b = dF/dp_M as gmpnp_galvanostat_terms returns it.
 * C and dI_r are the tangent's facet-wise functionals applied to Re x and Im x separately, the explicit d/dp_M part in the real part
 * alone; they are the sums over the wall (gmpnp_electrode_tangent's dD and dI of the p_M column at sigma = 0 and inv_dt = 0), a wall
 * mean divides them by sum_I w_I.  (K + i sigma M) x = -b is solved by a complex block-banded LU in the elimination order of the real
 * one (partial pivoting inside the 9 x 9 pivot blocks, key |re| + |im|), refined on the device by up to three rounds while the
 * residual max |(K + i sigma M) x + b| is above 1e-10 max |b| and halves.  The band, n (2 b + 1) 81 (re, im) pairs per frequency, is
 * storage of the response's own; frequencies go through the launches in chunks sized from gmpnp_options_t.band_lu_max_gb with one
 * host synchronisation per chunk.  A frequency's result does not depend on n or on the chunking, two calls give equal bits, and
 * afterwards F, the Jacobian, the real band LU, the status words and the validity flags are what they were, bit for bit.
 * status: bit 256 = a pivot block was singular, bit 512 = a value that is not finite, per frequency.
 * Refused (GMPNP_ERR_INVALID, the message names the frequency response): 1D handles (gmpnp_frequency_response), partition handles, a
 * coarse level attached or serving as one, the Stern option off, the galvanostat on, Stern and kinetic options with different
 * p_electrode, n outside 1 ... 4096, a sigma that is negative or not finite, a band of one frequency above band_lu_max_gb (the message
 * gives its size).  eps <= 0 on the wall or a rate that is not finite: GMPNP_ERR_NUMERIC.  gmpnp_time_kernel(30) times every launch
 * of the last chunk. */
int gmpnp_frequency_response_3d(gmpnp_solver* s, int32_t n, const double* sigma /* [n] */, gmpnp_response_t* out /* [n] */,
                                double* x_out /* [n][n_dofs][2] in file order, or NULL */);
/* The shape of a 3D handle's block-banded LU: the node blocks n and the stored band width b (the pattern's band in the elimination
 * order, at least 15: the substitution's panel).  The real factor takes n (2 b + 1) 81 doubles, the complex band of one frequency
 * twice that.  Nothing is allocated or launched. */
int gmpnp_band_lu_shape(gmpnp_solver* s, int32_t* n_blocks, int32_t* band);

/* ---- electrode tangent (no reference counterpart: polarisation curves by continuation in the electrode potential) --------------------
 * 1D and 3D handles with the Stern option on.  With p_M and the other electrode parameters theta_k as parameters of F(u; theta) = 0, the
 * tangent z_k = du/dtheta_k at the handle's current u, p_M and model.inv_dt solves
 *     J z_k = -c_k,   c_k = dF/dtheta_k
 * (inv_dt = 0: the tangent of the steady state; otherwise the tangent of one implicit step with u_n frozen).  Parameter codes:
 * 0 = p_M, 16 + r = ln k_r, 32 + r = alpha_r, 48 = ln lam (the Stern thickness).  The columns:
 *     p_M     gmpnp_galvanostat_terms' b, bit for bit (Stern rows g / lam, kinetic rows -w_I sum_r nu[r][i] alpha_r rate_r)
 *     ln k_r  +w_I nu[r][i] rate_r on the species rows            alpha_r  -w_I nu[r][i] rate_r (p_M - p_I - p_eq_r)
 *     ln lam  minus the Stern term of the potential rows (3D: per facet, in list order)          every Dirichlet row: 0
 * out[k] holds, for column k,
 *     dD = dD/dtheta + (dD/du).z       explicit part: g / lam for p_M, -D for ln lam, 0 otherwise (D = gmpnp_stern_displacement)
 *     dI_r = dI_r/dtheta + (dI_r/du).z explicit part: -alpha_r I_r for p_M, delta_rs I_r for ln k_s, -sum_I w_I rate_r (p_M - p_I - p_eq_r)
 *                                      for alpha_r, 0 for ln lam (I_r = gmpnp_kinetics_currents; 0 with the kinetics off)
 *     dp_boundary                      the w-weighted mean of z's potential entry over the Stern nodes
 *     residual                         max |J z + c| / max |c|
 *     status                           a word of that column alone: bit 1 = a value that is not finite
 * and z_out, where given, receives the tangents in file order.  F and J are assembled as the first iteration of gmpnp_newton_solve
 * assembles them; afterwards u, u_n, p_M and the model are untouched, F and J are those of the current u as after
 * gmpnp_assemble(want_jacobian = 1), and a following gmpnp_newton_solve gives the bits of a handle that never made the call.  3D: one
 * block-banded LU factorisation and n substitutions, each refined as the galvanostat's second column is, under band_lu_max_gb.  1D: the n
 * systems are solved by ONE block cyclic reduction of J that carries several right-hand sides (two or eight per chain): column k has
 * the bits of gmpnp_linear_solve(-c_k, GMPNP_LINEAR_BLOCK_TRIDIAGONAL), they do not depend on which other columns were asked for,
 * and two calls give equal bits.  eps <= 0 on the Stern boundary or a rate that is not finite at the state: GMPNP_ERR_NUMERIC.
 * gmpnp_tangent_columns: parity hook; the columns c_k of the last call, c_out[n][n_dofs] in file order.
 * gmpnp_electrode_advance is the predictor of a continuation in p_M: it needs a tangent whose p_M column was computed at the present
 * u, p_M and options (any call that changes one of them, a Newton solve included, invalidates it and the advance is refused), adds dp
 * to p_electrode of the Stern option and of the kinetic option, and sets u += alpha dp z_0 in one launch, compiled without fused
 * multiply-add (u + (alpha dp) z in IEEE double).  tau = 0: alpha = 1; otherwise alpha is the fraction-to-boundary factor of
 * gmpnp_step_limit for the direction -dp z_0, so that the state guess is damped while the potential takes the whole dp.  It marks the
 * Jacobian and the preconditioner invalid.
 * Refused (GMPNP_ERR_INVALID, the message names the electrode tangent): partition handles, a coarse level attached or
 * serving as one, SUPG terms set, the Stern option off, the galvanostat on, Stern and kinetic options with different p_electrode, a
 * kinetic parameter with the kinetics off or with r >= n_reactions, n outside 1 ... 10, a repeated or unknown parameter, a 1D handle
 * whose mesh does not serve the block-tridiagonal solver. */
#define GMPNP_TANGENT_MAX_COLUMNS 10
typedef struct {
  int32_t param;
  double dD;
  double dI[GMPNP_MAX_SURFACE_REACTIONS];
  double dp_boundary;
  double residual;
  int32_t status;                                /* 0, or bit 1 */
} gmpnp_tangent_t;
int gmpnp_electrode_tangent(gmpnp_solver* s, int32_t n, const int32_t* param /* [n] */, gmpnp_tangent_t* out /* [n] */,
                            double* z_out /* [n][n_dofs] in file order, or NULL */);
int gmpnp_tangent_columns(gmpnp_solver* s, double* c_out /* [n][n_dofs] in file order */);
int gmpnp_electrode_advance(gmpnp_solver* s, double dp, double tau, double* alpha_out /* or NULL */);

/* ---- parameter advance (no reference counterpart: the predictor of a fit of the electrode parameters to polarisation data) -----------
 * gmpnp_parameter_advance moves a 1D or 3D handle along several of the tangent's columns at once.  It needs a tangent computed at the
 * present u, p_M and options (whatever invalidates gmpnp_electrode_advance's tangent invalidates this one), every param[k] among the
 * parameters of that gmpnp_electrode_tangent call, its column's status 0.  A tangent call without a p_M column permits it in the columns
 * it did compute (gmpnp_electrode_advance stays refused after such a call).  Without fused multiply-add, every product and sum rounded
 * on its own, sums left to right in the order of THIS call's param:
 *     d = dtheta_0 z_0 + dtheta_1 z_1 + ...
 *     alpha = 1 (tau = 0), otherwise gmpnp_step_limit's factor for the direction -d
 *     u += (alpha dtheta_0) z_0 + (alpha dtheta_1) z_1 + ...
 * in one launch (tau = 0) or three (the direction, the limiter's partials, the update) and one host synchronisation; n = 1, param = {0}
 * gives gmpnp_electrode_advance's bits.  The parameters take the WHOLE step whatever alpha is: p_electrode += dtheta in both options,
 * k_r *= exp(dtheta), alpha_r += dtheta, lam *= exp(dtheta) (exp of the host's C library); the moved options are validated by the rules
 * of gmpnp_set_stern and gmpnp_set_kinetics before anything is changed.  On success the Jacobian and the preconditioner are marked
 * invalid and the tangent is dropped.  A direction that is not finite (tau != 0): nothing is applied, GMPNP_ERR_NUMERIC, the tangent is
 * dropped.  Refused (GMPNP_ERR_INVALID, the message names the parameter advance; u, the options and the tangent stay as they were):
 * everything gmpnp_electrode_tangent refuses of a handle, n outside 1 ... 10, a repeated parameter, a parameter not in the last tangent
 * call, a dtheta that is not finite, tau outside {0} and (0, 1), a stale or missing tangent, moved options that are not valid.
 * gmpnp_get_electrode_options: the handle's current option structs (p_electrode is the galvanostat's p_M while it is on; model = 0 /
 * n_reactions = 0 and zeros while an option is off).  It launches nothing and changes nothing. */
int gmpnp_parameter_advance(gmpnp_solver* s, int32_t n, const int32_t* param /* [n] */, const double* dtheta /* [n] */,
                            double tau, double* alpha_out /* or NULL */);
int gmpnp_get_electrode_options(gmpnp_solver* s, gmpnp_stern_t* stern_out /* or NULL */, gmpnp_kinetics_t* kinetics_out /* or NULL */);

/* ---- potential programmes (no reference counterpart: the electrode potential follows a waveform in time; rule: "potential programmes"
 * in csrc/gmpnp_host_rules.h and gmpnp_amd/programme.py; kernels: csrc/gmpnp_trace.h) -------------------------------------------------
 * gmpnp_set_electrode_potential: p_electrode of the Stern option and, where the kinetics are on, of the kinetic option become p, in one
 * call with one synchronisation.  It drops the tangent, marks the Jacobian and the preconditioner invalid and rebinds the boundary
 * vector once; afterwards F, J and gmpnp_get_electrode_options hold the bits that gmpnp_set_stern followed by gmpnp_set_kinetics with
 * that value give.  Refused (GMPNP_ERR_INVALID, the message names the electrode potential): the Stern option off, the galvanostat on,
 * p not finite.
 *
 * The electrode trace is a per-handle buffer of records that the device fills, one per accepted time step, allocated by the first
 * gmpnp_electrode_trace_open (a handle that never asks keeps the buffers and launches it had).
 *   open(capacity)    allocates `capacity` slots, resets the count, evaluates D at the current u as D_prev and zeroes Q and Q_D
 *                     (one synchronisation)
 *   append(t, h)      k_stern_residual, k_kinetics_residual (kinetics on) and k_electrode_record at the current u, which writes the
 *                     next slot: no host synchronisation and no copy.  With w_I the weights of the kinetics (1D: 1, 3D: the wall
 *                     weights) over the nodes of the Stern boundary:
 *                         D            the bits of gmpnp_stern_displacement          I[r]   the bits of gmpnp_kinetics_currents
 *                         p_boundary   sum_I w_I p_I / sum_I w_I                            (0 with the kinetics off)
 *                         u_boundary   sum_I w_I u_{I,f} / sum_I w_I per species (0 behind the handle's species)
 *                         dD_dt = (D - D_prev) / h     Q[r] += h I[r]     Q_D += h dD_dt     D_prev = D
 *                     every product, quotient and sum of the last line rounded on its own (electrode_record_combine of the rule; the
 *                     device keeps D_prev, Q and Q_D).  status bit 1: a value of the record is not finite.  A full buffer is refused
 *                     and nothing is overwritten: read the records and open again, or open with more room.
 *   read(first, n)    records first ... first + n - 1 with one synchronisation and one copy
 *   close()           the trace is closed (the buffer stays with the handle); append, read and hook 29 are refused until the next open
 * Refused (GMPNP_ERR_INVALID, the message names the electrode trace): the Stern option off, partition handles, a multilevel coarse
 * level attached or the handle serving as one, the galvanostat on, capacity < 1, h <= 0 or not finite, t not finite, append / read /
 * close without an open trace, a read outside the records written. */
typedef struct {
  double t, h;                                /* the arguments of the append */
  double p_M;                                 /* p_electrode of the Stern option */
  double p_boundary;
  double D, dD_dt;
  double I[GMPNP_MAX_SURFACE_REACTIONS];
  double Q[GMPNP_MAX_SURFACE_REACTIONS];
  double Q_D;
  double u_boundary[GMPNP_MAX_SPECIES];
  int32_t status;                             /* bit 1: a value that is not finite */
  int32_t pad_;
} gmpnp_electrode_record_t;
int gmpnp_set_electrode_potential(gmpnp_solver* s, double p);
int gmpnp_electrode_trace_open(gmpnp_solver* s, int32_t capacity);
int gmpnp_electrode_trace_append(gmpnp_solver* s, double t, double h);
int gmpnp_electrode_trace_read(gmpnp_solver* s, int32_t first, int32_t n, gmpnp_electrode_record_t* out /* [n] */);
int gmpnp_electrode_trace_close(gmpnp_solver* s);

/* ---- wall profile (no reference counterpart: the electrode record resolved along the axis of the 3D pore; rule: "wall profile" in
 * csrc/gmpnp_host_rules.h and gmpnp_amd/programme.py; kernel: csrc/gmpnp_wall_profile.h) ---------------------------------------------
 * 3D handles.  The nodes of the Stern boundary (the wall) are sorted into n_bins axial bins by their z, the mesh's third coordinate in
 * units of L: edges[n_bins + 1] finite and strictly ascending, the bin of z the largest b with edges[b] <= z, z == edges[n_bins] in
 * the last bin, z outside the edges in no bin (wall_bin of the rule; a node on an interior edge is counted once).  The profile is a
 * per-handle buffer of capacity x n_bins records that the device fills, n_bins per accepted time step, allocated by the first
 * gmpnp_wall_profile_open (a handle that never asks keeps the buffers and launches it had).
 *   open(n_bins, edges, capacity)   sorts the nodes, uploads the lists, allocates capacity x n_bins slots, resets the count and zeroes
 *                     the charges Q of every bin (one synchronisation).  A bin without a node is refused and the message names it:
 *                     ask for fewer bins.
 *   append(t, h)      k_stern_residual, k_kinetics_residual (kinetics on) and k_wall_profile (one workgroup per bin) at the current
 *                     u, which writes the step's n_bins slots: no host synchronisation and no copy.  Over the nodes I of bin b, in the
 *                     statements and the order of gmpnp_electrode_trace_append's record, with w_I the wall weights:
 *                         area = sum_I w_I     D = sum_I (Stern term of the potential row)     I[r] = sum_I w_I rate_r (0 with the
 *                         kinetics off)       p_mean = sum_I w_I p_I / area     u_mean[f] = sum_I w_I u_{I,f} / area
 *                         Q[r] += h I[r]      (product and sum rounded on their own; the device keeps Q per bin)
 *                     With one bin over the whole wall D and I are the bits of gmpnp_electrode_record_t.  status bit 1: a value of the
 *                     bin's record is not finite (the other bins are not touched).  No floating-point atomics: two profiles of one
 *                     sequence of states give equal bits.  A full buffer is refused and nothing is overwritten.
 *   read(first, n)    the records of steps first ... first + n - 1, out[n][n_bins], one synchronisation and one copy
 *   close()           append, read and hook 32 are refused until the next open (the buffers stay with the handle)
 * Refused (GMPNP_ERR_INVALID, the message names the wall profile): 1D handles (the electrode record is their profile), the Stern option
 * off, partition handles, a multilevel coarse level attached or the handle serving as one, the galvanostat on, n_bins outside
 * 1 ... 256 or edges that are not finite and strictly ascending, a bin without a node, capacity < 1, h <= 0 or not finite, t not
 * finite, append / read / close without an open profile, a read outside the steps written, a full buffer. */
#define GMPNP_WALL_PROFILE_MAX_BINS 256
typedef struct {
  double t, h;                                /* the arguments of the append */
  double z_lo, z_hi;                          /* the bin's edges */
  double area;                                /* sum of the wall weights of the bin's nodes (scaled units) */
  double D;
  double I[GMPNP_MAX_SURFACE_REACTIONS];
  double Q[GMPNP_MAX_SURFACE_REACTIONS];
  double p_mean;
  double u_mean[GMPNP_MAX_SPECIES];
  int32_t count;                              /* nodes of the bin */
  int32_t status;                             /* bit 1: a value that is not finite */
} gmpnp_wall_profile_record_t;
int gmpnp_wall_profile_open(gmpnp_solver* s, int32_t n_bins, const double* edges /* [n_bins + 1] */, int32_t capacity);
int gmpnp_wall_profile_append(gmpnp_solver* s, double t, double h);
int gmpnp_wall_profile_read(gmpnp_solver* s, int32_t first, int32_t n, gmpnp_wall_profile_record_t* out /* [n][n_bins] */);
int gmpnp_wall_profile_close(gmpnp_solver* s);

/* ---- transient sensitivities (no reference counterpart: what a marched potential programme says about the electrode parameters;
 * kernels: csrc/gmpnp_sensitivity.h) ---------------------------------------------------------------------------------------------------
 * 1D handles.  With J = K + inv_dt M (M the consistent P1 mass on the free species rows) the backward-Euler time term is linear in u_n,
 * dF/du_n = -inv_dt M, so the exact discrete forward sensitivity s_k = du/dtheta_k of a marched programme obeys, per accepted step,
 *     J(u^{n+1}) s_k^{n+1} = -c_k(u^{n+1}) + inv_dt M s_k^n          (Dirichlet rows: 0)
 * with the electrode tangent's columns c_k = dF/dtheta_k and its parameter codes (0 = p_M: an offset of the whole waveform, 16 + r =
 * ln k_r, 32 + r = alpha_r, 48 = ln lam).  The buffers are per handle and allocated by the first gmpnp_sensitivity_open (a handle that
 * never asks keeps the buffers and launches it had).
 *   open(n, param, start, capacity)   n = 1 ... 10 columns and a record buffer of `capacity` steps x n columns.  start = 0: S = 0 (the
 *                     state the march starts from does not depend on theta); start = 1: S = the columns of a still-valid
 *                     gmpnp_electrode_tangent call that holds every param[k] with status 0 (made at inv_dt = 0 it is the steady state's
 *                     dependence on theta; refused with a stale or missing tangent, as gmpnp_parameter_advance is); start = 2: S and
 *                     the accumulators stay what they are and only the count is reset (the same n and param as the open before: a
 *                     full buffer was read).  start 0 and 1 take the tangent's functional dD of S at the current u and options as
 *                     dD_prev and zero dQ and dQ_D.  One synchronisation.
 *   step(t, h)        once per accepted step, after its Newton solve, with model.inv_dt the step's; u_n is not read.  It enqueues its
 *                     launches and returns: no host synchronisation, no copy.  F and J are assembled at the current u as
 *                     gmpnp_electrode_tangent assembles them and the columns c_k are formed by its kernels; k_sens_rhs writes
 *                     -c_k + inv_dt M s_k straight into level 0 of the multi-column cyclic reduction (at most 2 columns: one chain of
 *                     2; otherwise a chain of 8 and, for columns 9 and 10, a chain of 2); the solution replaces S; k_sens_record (one
 *                     workgroup, fixed order, no floating-point atomics) applies the tangent's functionals to S and the trace's combine
 *                     step to the derivatives, every product, quotient and sum rounded on its own,
 *                         d_dD_dt = (dD - dD_prev) / h     dQ[r] += h dI[r]     dQ_D += h d_dD_dt     dD_prev = dD
 *                     and stores one record per column.  status: bit 1 = a value of the column that is not finite, bit 2 = the
 *                     elimination met a singular pivot, bit 4 = the assembly reported eps <= 0 or a rate that is not finite.
 *                     Afterwards u, u_n, the options and the electrode trace are untouched, F and J are those of the current u, a
 *                     following gmpnp_newton_solve gives the bits of a handle that never made the call, and the tangent is dropped as
 *                     after a tangent call.  A column's records and S do not depend on which other columns are carried; two runs give
 *                     equal bits; from start = 0 the first step is gmpnp_electrode_tangent at that state and inv_dt, bit for bit.
 *                     A full buffer is refused and nothing is overwritten: read the records and open with start = 2.
 *   read(first, n_steps)   the records of steps first ... first + n_steps - 1, out[n_steps][n], one synchronisation and one copy
 *   columns(which)    parity hook: which = 0 the sensitivities S, which = 1 the right-hand sides of the last step, out[n][n_dofs] in
 *                     file order
 *   close()           step, read, columns and hook 31 are refused until the next open (the buffers stay with the handle)
 * Refused (GMPNP_ERR_INVALID, the message names the sensitivities): everything gmpnp_electrode_tangent refuses of a handle, 3D handles,
 * n outside 1 ... 10, an unknown or repeated parameter, a kinetic parameter with the kinetics off or of a reaction >= n_reactions,
 * capacity < 1, start outside 0 ... 2, start = 2 without an earlier open of the same columns, h <= 0 or not finite, t not finite, step /
 * read / columns / close without an open buffer, a read outside the steps written. */
typedef struct {
  double t, h;                                /* the arguments of the step */
  int32_t param;
  int32_t pad0_;
  double dD, d_dD_dt;
  double dI[GMPNP_MAX_SURFACE_REACTIONS];
  double dQ[GMPNP_MAX_SURFACE_REACTIONS];
  double dQ_D;
  double dp_boundary;
  double residual;                            /* max |J s - rhs| / max |rhs| */
  int32_t status;                             /* bits 1, 2, 4 */
  int32_t pad_;
} gmpnp_sensitivity_record_t;
int gmpnp_sensitivity_open(gmpnp_solver* s, int32_t n, const int32_t* param /* [n] */, int32_t start, int32_t capacity);
int gmpnp_sensitivity_step(gmpnp_solver* s, double t, double h);
int gmpnp_sensitivity_read(gmpnp_solver* s, int32_t first, int32_t n_steps, gmpnp_sensitivity_record_t* out /* [n_steps][n] */);
int gmpnp_sensitivity_columns(gmpnp_solver* s, int32_t which, double* out /* [n][n_dofs] in file order */);
/* Parity hook's counterpart: S <- in (what the tests of the right-hand side and of the status word plant); dD_prev, dQ and dQ_D stay. */
int gmpnp_sensitivity_set_columns(gmpnp_solver* s, const double* in /* [n][n_dofs] in file order */);
int gmpnp_sensitivity_close(gmpnp_solver* s);

/* ---- periodic steady state: the accelerated cycle map (no reference counterpart: the limit cycle of a potential programme; kernels:
 * csrc/gmpnp_cycle.h; rules: anderson_weights and cycle_verdict of csrc/gmpnp_host_rules.h; driver: gmpnp_amd/periodic.py; DESIGN.md
 * section 5r) ----------------------------------------------------------------------------------------------------------------------------
 * The cycle map Phi takes u_n at the start of one period of a waveform, marched with fixed steps, to u_n at its end.  The handle keeps a
 * window of at most depth + 1 pairs (x_j, g_j = Phi(x_j)), oldest first, k the newest, and one weight vector.  With r_j = g_j - x_j and
 * d_j = r_{j+1} - r_j, Anderson acceleration (type II, beta = 1) takes theta = argmin |r_k - sum_j theta_j d_j|_W and goes on from
 * x_{k+1} = g_k - sum_j theta_j (g_{j+1} - g_j) = sum_j gamma_j g_j, sum_j gamma_j = 1.  The device forms the residual norm and the
 * normal system, the host solves it (anderson_weights) and the device mixes the stored states.
 *   open(depth, tol)  depth 1 ... 8; allocates depth + 1 pairs of n_dofs doubles and the weights, frozen HERE from the current u_n:
 *                     w = atol_f + rtol |u_n| per dof.  Empties the window.  One synchronisation.
 *   begin()           x_k <- u_n (a device copy); the oldest pair leaves a full window
 *   end(report)       g_k <- u_n, the pair enters the window; over the dofs that carry no Dirichlet value (a Dirichlet dof's change
 *                     over a cycle is boundary data):
 *                         err = sqrt(sum (r_k / w)^2 / n_free)     err_max = max |r_k / w| at worst_dof (ties: the smaller dof of
 *                         the handle's internal order)             A_ij = sum (d_i / w)(d_j / w)     b_i = sum (d_i / w)(r_k / w)
 *                     for i, j < window - 1, zero behind; the differences are formed first and then the products (a Gram matrix of
 *                     the r_j would cancel where successive residuals agree to several digits).  A NaN / Inf anywhere in a stored
 *                     vector of the window or in the weights (u_n was not finite at the open) sets nonfinite and makes err and
 *                     err_max NaN; the status stays GMPNP_OK, and a mix behind such a report is refused (with tau = 0 no pass of
 *                     the mix would notice the value on its way into u and u_n): restart, or open again.  Fixed-order
 *                     reductions, no atomics: two calls on one window return the same bits.  One synchronisation.
 *   mix(n, gamma, tau, alpha_out)   n = the window of the last report, every gamma finite, |sum gamma - 1| <= 1e-12 (summed left to
 *                     right).  Free rows: u = u_n <- g_k + alpha (sum_j gamma_j g_j - g_k), the sum over j in window order from
 *                     gamma_0 g_0, every product and sum rounded on its own; Dirichlet rows: g_k.  alpha = 1 with tau = 0, otherwise
 *                     the fraction-to-boundary factor of gmpnp_step_limit for the correction dx = -(sum_j gamma_j g_j - g_k) at the
 *                     state g_k (the same kernel and rule).  A NaN / Inf in that direction: nothing is applied, alpha = NaN,
 *                     GMPNP_ERR_NUMERIC.  Afterwards the handle is where gmpnp_set_state(u, u) leaves it: no history levels, the
 *                     state marked as set from outside, Jacobian and preconditioner invalid, the tangent dropped, the time term
 *                     reading u_n.  A second mix needs another end.
 *   restart()         empties the window (the weights stay)
 *   vectors(which, out)   parity hook, file order: which = 0 the x_j, 1 the g_j ([window][n_dofs], window order), 2 the weights
 *   close()           every call but open is refused until the next open (the buffers stay with the handle)
 * Everything is allocated by the first open: a handle that never calls it keeps the buffers and launches it had.  Refused
 * (GMPNP_ERR_INVALID, the message names the cycle): partition handles, a coarse level attached or the handle serving as one, the
 * galvanostat on, order-2 time stepping (p_M, u_nm1 would be part of the map's state), depth outside 1 ... 8, a tolerance
 * gmpnp_time_error would refuse, any call but open without an open cycle, end without begin, mix before end or behind a report with nonfinite set, a wrong n, a gamma that is
 * not finite or does not sum to 1, tau outside {0} and (0, 1), and at mix an open electrode trace, sensitivity session or wall profile
 * (close them and open them again behind the mix: their accumulators then start at the mixed state). */
#define GMPNP_CYCLE_MAX_DEPTH 8
typedef struct {
  double err, err_max;
  int64_t worst_dof;                                             /* file order (vertex*n_fields+field), -1: none */
  int64_t n_free;
  int32_t nonfinite, window;                                     /* window: pairs held, this one included */
  double A[GMPNP_CYCLE_MAX_DEPTH * GMPNP_CYCLE_MAX_DEPTH];       /* row-major, both triangles filled from the upper one */
  double b[GMPNP_CYCLE_MAX_DEPTH];
} gmpnp_cycle_report_t;
int gmpnp_cycle_open(gmpnp_solver* s, int32_t depth, const gmpnp_time_tol_t* tol);
int gmpnp_cycle_begin(gmpnp_solver* s);
int gmpnp_cycle_end(gmpnp_solver* s, gmpnp_cycle_report_t* report);
int gmpnp_cycle_mix(gmpnp_solver* s, int32_t n, const double* gamma /* [n] */, double tau, double* alpha_out /* or NULL */);
int gmpnp_cycle_restart(gmpnp_solver* s);
int gmpnp_cycle_vectors(gmpnp_solver* s, int32_t which, double* out);
int gmpnp_cycle_close(gmpnp_solver* s);

/* ---- ensemble of problems (no reference counterpart: the reference solves one problem per run; a voltage x cation x
 * concentration sweep of 1D/MPNP_CO2ER_EDL.py or 3D/MPNP_CO2ER_pore.py is many separate runs) ------------------------------------
 * n = 1 ... 64 handles the caller made with gmpnp_create on the SAME mesh (same vertices, cells and vertex order) and device,
 * all of them 1D or all of them 3D.
 * Each member keeps its whole per-handle surface (gmpnp_set_model, gmpnp_set_dirichlet, gmpnp_set_state / gmpnp_get_state,
 * gmpnp_project_gradient / gmpnp_project_cellwise) and its own model tables, Dirichlet values and state; the ensemble only runs
 * the Newton iterations of all members in one launch chain per iteration (one host synchronisation per iteration for the
 * whole ensemble).  Refused (GMPNP_ERR_INVALID, the message names the member and the reason): 1D and 3D handles together,
 * partitioned handles, members on other devices or with another topology, SUPG terms set on a member, n outside 1 ... 64; every
 * condition is checked again at every solve.
 * A 3D member (8 species + potential) is created with gmpnp_options_t.shared_device = 1 (one stream, four launches per BiCGStab
 * iteration: nothing waits inside a launch) and is refused with a multilevel coarse level attached, in the materialised vector
 * form (vector_form 1), with progress_by_copy, or on a mesh with more than 128 tile slots per aggregate.  Per Newton iteration
 * the Jacobian gather, the preconditioner set-up, the test of the predicted start, the first BiCGStab pass, the final M^-1
 * application with the Newton update and the next residual run as one launch chain for all members; a member whose linear solve
 * leaves that path (first pass not converged within 500 iterations, breakdown, iteration cap, band LU due) is finished by the
 * single handle's code for that iteration while the others wait, and joins again at the next residual.
 * The members stay owned by the caller and must outlive the ensemble.  Every ensemble call is complete when it returns: a
 * member call made afterwards on the member's own stream sees the ensemble's results. */
typedef struct gmpnp_ensemble gmpnp_ensemble;
int gmpnp_ensemble_create(int32_t n, gmpnp_solver* const* members, gmpnp_ensemble** out);
void gmpnp_ensemble_destroy(gmpnp_ensemble* e);
int32_t gmpnp_ensemble_size(const gmpnp_ensemble* e);
/* solve(F == 0, u, bcs, solver_parameters) on every member at once; opts.linear_solver must be GMPNP_LINEAR_BLOCK_TRIDIAGONAL for
 * 1D members and GMPNP_LINEAR_BICGSTAB_TWOLEVEL or GMPNP_LINEAR_BICGSTAB_JACOBI for 3D members (GMPNP_LINEAR_BAND_LU is refused).
 * stats[n] and status[n] (a gmpnp_status per member) are what gmpnp_newton_solve on that handle alone returns, timing fields
 * excepted; a member that has converged or failed gets no further updates while the others go on.  Returns 0 when every member
 * succeeded, else the first non-zero member status (gmpnp_last_error names the member). */
int gmpnp_ensemble_newton_solve(gmpnp_ensemble* e, const gmpnp_newton_options_t* opts, gmpnp_newton_stats_t* stats, int32_t* status);
/* Message of member k's failure in the last gmpnp_ensemble_newton_solve ("" = none). */
const char* gmpnp_ensemble_member_error(const gmpnp_ensemble* e, int32_t k);
/* u_n.assign(u) on every member (blocking). */
int gmpnp_ensemble_assign_previous(gmpnp_ensemble* e);
/* u of every member, u_out[n][n_dofs] in file order, with one device-to-host copy for the whole ensemble. */
int gmpnp_ensemble_get_state(gmpnp_ensemble* e, double* u_out);
/* Adaptive time stepping of the members, every member with its own step size (the batched forms of gmpnp_set_time_step,
 * gmpnp_time_error, gmpnp_time_accept and gmpnp_time_reject; kernels: csrc/gmpnp_time_step_ens.h).  u_nm1 and the estimator's
 * storage are the member's own, so the history is shared with the single-handle calls: after an accept here gmpnp_time_error on
 * the member sees it, and the other way round.  All three check the members' configuration again as gmpnp_ensemble_newton_solve
 * does, and are complete when they return.
 * set_time_step: inv_dt[k] becomes member k's model.inv_dt on the host and the device, its Jacobian and preconditioner are
 * invalidated; one synchronisation for the whole ensemble.  Every value is validated first by gmpnp_set_time_step's rule: a bad one
 * is GMPNP_ERR_INVALID, the message names the member, and nothing is changed.
 * time_error: gmpnp_time_error of every listed member (mask[k] != 0; NULL = all) with its own h[k], h_prev[k] and tol[k], in two
 * launches and one host synchronisation.  The arguments of a listed member are validated as gmpnp_time_error validates them (the
 * message names the member).  out[k] holds, bit for bit, what gmpnp_time_error on member k alone returns; has_history is the
 * member's.  The row of a member that is not listed is zeroed and its estimator storage is not written.  A NaN / Inf in one
 * member's u sets that member's nonfinite and err values and leaves the other rows as they are.
 * time_advance: action[k] = 0 leaves member k alone, 1 accepts its step (u_nm1 <- u_n, u_n <- u, has_history = 1), 2 rejects it
 * (u <- u_n; the next Newton solve starts from a state set from outside), in one launch.  Any other value is GMPNP_ERR_INVALID
 * and nothing is launched. */
int gmpnp_ensemble_set_time_step(gmpnp_ensemble* e, const double* inv_dt /* [n] */);
int gmpnp_ensemble_time_error(gmpnp_ensemble* e, const double* h /* [n] */, const double* h_prev /* [n] */, const gmpnp_time_tol_t* tol /* [n] */,
                              const int32_t* mask /* [n], NULL = all */, gmpnp_time_error_t* out /* [n] */);
int gmpnp_ensemble_time_advance(gmpnp_ensemble* e, const int32_t* action /* [n]: 0 leave, 1 accept, 2 reject */);

/* Benchmark hooks: time `launches` back-to-back launches of one kernel on the handle's stream with HIP
 * events; kernel: 0 = plain Jacobian SpMV, 1 = element kernel (F+J), 2 = Jacobian gather, 3 = residual gather,
 * 4/5 = fused BiCGStab half-iterations A/B, 6/7 = their scalar+coarse kernels, 8 = one-wave copy, 9-11 = streaming
 * read of the matrix buffer with 2048 / 512 / 8192 workgroups (bandwidth probes), 12/13 = the two-launch form of the
 * half-iterations (coarse workgroups inside the tile launch), 14/15 = the tile kernels of the materialised vector form,
 * 16/17 = its streaming vector updates, 18 = one whole 1D direct solve (block cyclic reduction: extraction, every level down
 * and up; needs an assembled Jacobian), 19 = element kernel without J (with 3: one residual evaluation), 20 = the launch chain of one
 * gmpnp_species_budget call (element kernel without J, cell pass, row pass, final sums), 21 = the two launches of the step limiter
 * (k_step_limit + k_limited_update, on a zero correction: the state stays), 22 = the three launches of an accepted adaptive time step
 * (estimator + reduce + shift; u_n and u_nm1 are put back afterwards, the history flag stays), 23 = the four launches of an accepted
 * order-2 step (u*, order-2 estimator, reduce, three-deep shift; u_n, u_nm1 and u_nm2 are put back, the order and the levels stay;
 * allocates the order-2 vectors), 24 = the two launches of the Stern boundary condition (k_stern_residual + k_stern_jacobian; needs
 * gmpnp_set_stern with model != 0 and an assembled Jacobian, which the launches keep adding to), 25 = the two launches of the surface
 * kinetics (k_kinetics_residual + k_kinetics_jacobian; needs gmpnp_set_kinetics with n_reactions > 0 and an assembled Jacobian, which
 * the launches keep adding to), 26 = the galvanostat's launches of one Newton iteration apart from the two linear solves (k_galv_rhs,
 * k_galv_reduce, k_galv_direction, k_galv_potential on a zero step, k_galv_reduce for G alone; needs gmpnp_set_galvanostat with on != 0
 * and an assembled Jacobian; the state and p_M stay), 27 = the two launches of one chunk of the frequency response (k_response_solve +
 * k_response_functional on the frequencies of the last chunk of the last gmpnp_frequency_response call, which it needs), 28 = the
 * multi-column cyclic-reduction chain(s) of the last gmpnp_electrode_tangent call with extraction and application (needs such a call
 * and the Jacobian it left), 29 = the launches of one gmpnp_electrode_trace_append (k_stern_residual, k_kinetics_residual with the
 * kinetics on, k_electrode_record; needs an open trace, whose records, count, D_prev, Q and Q_D stay: the hook's launches write a slot
 * and accumulators of their own), 30 = every launch of one chunk of the 3D frequency response (scatter, k_cband_step per pivot, the
 * solve and its refinement rounds, k_cband_functional on the frequencies of the last chunk of the last gmpnp_frequency_response_3d
 * call, which it needs; it writes the response's own storage only), 31 = the launches of one gmpnp_sensitivity_step (assembly, columns,
 * k_sens_rhs, the multi-column chain(s), application, k_spmv_plain per column, k_sens_record; needs an open sensitivity buffer, whose S,
 * records, count and accumulators stay: the hook's launches work on a second S (allocated by the first hook call), a slot and
 * accumulators of their own; like a step it reassembles F and J at the current u and drops the tangent, so a gmpnp_sensitivity_open with
 * start = 1 needs a gmpnp_electrode_tangent call made after it), 32 = the launches of one gmpnp_wall_profile_append (k_stern_residual,
 * k_kinetics_residual with the kinetics on, k_wall_profile; needs an open wall profile, whose records, count and charges stay: the
 * hook's launches write the row of slots behind the buffer and charges of their own), 33 = the launches of one cycle residual and
 * one mix (k_cycle_residual, k_cycle_reduce, then k_cycle_mix's direction pass, k_step_limit and k_cycle_mix's apply pass with
 * gamma = the newest pair alone and tau = 0.9; needs an open cycle with at least one pair behind a gmpnp_cycle_end; u and u_n are put
 * back, the window, the history and the handle's flags stay). */
int gmpnp_time_kernel(gmpnp_solver* s, int32_t kernel, int32_t launches, double* avg_us);
/* Fused BiCGStab half-iterations (SpMV + vector updates) timed with HIP events since the last call (opts.profile_every):
 * n_sampled = half-iterations inside the timed bursts (each a run of back-to-back launches, all of them before the end of
 * their solve), mean_us = elapsed time / n_sampled (launch gaps included), n_launched = all half-iterations launched. */
int gmpnp_spmv_profile(gmpnp_solver* s, int64_t* n_sampled, double* mean_us, int64_t* n_launched);
/* Mean elapsed time of an EMPTY event pair on the handle's stream (what a sampled launch's bracket adds). */
int gmpnp_event_overhead(gmpnp_solver* s, int32_t pairs, double* mean_us);

#ifdef __cplusplus
}
#endif
#endif /* GMPNP_H */
