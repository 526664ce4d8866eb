/*
 * dto_engine.h -- C ABI of the MI355X-native NLP-callback engine for DirectTrajOpt.jl.
 *
 * Drop-in boundary: the seven MOI.AbstractNLPEvaluator methods implemented by the reference's
 * `Evaluator` (src/solvers/evaluator.jl:66-98, 291-456).  A Julia shim `GPUEvaluator <:
 * MOI.AbstractNLPEvaluator` forwards each MOI method to one entry point below through `@ccall`
 * (see INTEGRATION.md).  Plain C: pointers + sizes only, no exceptions cross the boundary.
 *
 * Conventions
 *   - All floating-point data are IEEE double; all index outputs are int64, 1-BASED (Julia/MOI).
 *   - Matrices are dense COLUMN-MAJOR (Julia's native layout).
 *   - The NLP variable vector is Z = [datavec; global_data], datavec knot-major
 *     (src/solvers/evaluator.jl:230, 474-482); component offsets are 0-based inside a knot.
 *   - Return value 0 = OK, non-zero = error; text via dto_last_error().  A kernel launch the HIP runtime rejects
 *     (hipGetLastError after the call's launches) is such an error.  Errors that only show once the device has
 *     run -- a generator sweep that exhausted its step budget -- are reported by the blocking entry points at once,
 *     and by the `*_dev` entry points on the NEXT call through the ABI on that handle (any entry point, including
 *     dto_last_stats, which synchronises): that call returns non-zero without doing its own work and clears the flag.
 *   - One in-flight call per handle (solvers call back serially).
 *   - `*_dev` entry points take DEVICE pointers and a hipStream_t (passed as void*); inputs and outputs
 *     stay in HBM and the call returns with the last kernels still in flight on `stream`.  They may wait
 *     on a few 8-16 byte device-to-host readbacks in between (data-dependent launch counts: squarings,
 *     Taylor terms), so they are not graph-capturable.  The plain entry points take HOST pointers, copy
 *     in/out and block until the result is in the caller's buffer.
 *   - A handle may own a SHARD of the knot range [k_lo, k_hi] (1-based, inclusive).  All value
 *     outputs are then the shard-local contiguous slabs described by dto_shard_info; with
 *     k_lo = 1, k_hi = N the slabs are the whole vectors.
 */
#ifndef DTO_ENGINE_H
#define DTO_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTO_ABI_VERSION 8

/* integrator kinds (src/integrators/) */
#define DTO_INTEGRATOR_BILINEAR 1   /* bilinear_integrator.jl:61-85   */
#define DTO_INTEGRATOR_DERIVATIVE 2 /* derivative_integrator.jl:26-49 */
#define DTO_INTEGRATOR_EXTERNAL 3   /* any other AbstractIntegrator (TimeDependentBilinearIntegrator,
                                       time_dependent_bilinear_integrator.jl:60-244; user integrators): evaluated
                                       on the HOST by the reference's own code, merged by the engine.  Structure is
                                       the generic one (dense x_dim x 2z block per interval, _integrators.jl:49-77);
                                       only x_dim is read from the descriptor */

#define DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR 4 /* TimeDependentBilinearIntegrator (time_dependent_bilinear_integrator.jl:
                                       60-244) for the parametrised generator family
                                         G(u, t) = sum_{j=0..m} ubar_j ( G_j + sum_c phi_c(t) H_cj ),  ubar_0 = 1,
                                         phi_c(t) = cos(omega_c t) or sin(omega_c t)
                                       (carrier-modulated drives, rotating-frame terms; the reference's own test
                                       G(a) + 0.1 cos(t) I is the case H_c0 = 0.1 I).  Evaluated ON THE DEVICE: defect
                                       x_{k+1} - Phi_k x_k of  dx/dtau = dt_k G(u(tau), t_k + tau dt_k) x,  tau in [0,1], by
                                       classical RK4 with `substeps` fixed steps (the reference integrates adaptively with
                                       Tsit5), controls held (spline_order 0) or interpolated linearly to u_{k+1} (1), with the
                                       exact first and second derivatives of that discrete map.  Device range: 0..7 drives, 1..256 states
                                       (1..64: a scalar kernel; 65..256: FP64 matrix-core products), substeps >= 1, and a
                                       coefficient table (1 + p + p (p+1) / 2) (m+1) (1 + n_mod) <= 6144 with
                                       p = m + 2 (+ m for spline_order 1); dto_create refuses anything else and names the
                                       limit.  With DTO_FLAG_BLOCK_GENERATORS a family of replicated blocks (every G_j and
                                       H_cj == I_r (x) B, r >= 2, blocks of at most 64 rows) runs on the blocks at 33..512
                                       states.  An arbitrary closure G(u, t) stays DTO_INTEGRATOR_EXTERNAL */

/* objective term kinds (src/objectives/) */
#define DTO_OBJECTIVE_QUADRATIC_REGULARIZER 1 /* regularizers.jl:38-167   */
#define DTO_OBJECTIVE_LINEAR_REGULARIZER 2    /* regularizers.jl:207-313  */
#define DTO_OBJECTIVE_MINIMUM_TIME 3          /* minimum_time_objective.jl:24-76 */
#define DTO_OBJECTIVE_KNOT_SQDIST 4           /* KnotPointObjective / TerminalObjective with the built-in loss
                                                 l(v, p) = ||v - p||^2 (knot_point_objectives.jl:65-243) */
#define DTO_OBJECTIVE_KNOT_LOWRANK_INFIDELITY 6 /* KnotPointObjective / TerminalObjective with the built-in loss
                                                 l(v) = |1 - ||A v||^2|, A a constant k x n_comps factor: the
                                                 coherent (ket / unitary) fidelity losses in isomorphic
                                                 coordinates, whose per-knot Hessian is the ConstantLowRankHVP
                                                 shape A' G A with G = -2 sign(1 - F) I (knot_hvp.jl:45-84).
                                                 A is passed in `R` (k x n_comps column-major), k in `comp_dim` */
#define DTO_OBJECTIVE_EXTERNAL_GLOBAL 7         /* GlobalObjective / GlobalKnotPointObjective (global_objectives.jl:35-350),
                                                 host closure over [z_t[comps]; global_data[gcomps]] per listed time
                                                 (n_times = 0: one listing of the global variables alone).  Gradient
                                                 and Hessian blocks ACCUMULATE over the listings (:270-271, :341), the
                                                 Hessian entries whose column is a global variable form the tail of
                                                 the CSC order (global columns follow all knot columns) */
#define DTO_OBJECTIVE_EXTERNAL_KNOT 5         /* KnotPointObjective / TerminalObjective with a HOST closure l: the
                                                 caller evaluates Q_i l, its gradient and Hessian per listed time
                                                 (the reference's own ForwardDiff code, knot_point_objectives.jl:
                                                 173-243) and hands the blocks over with dto_set_external; the
                                                 engine merges them at its precomputed offsets */

/* built-in g kinds for NonlinearKnotPointConstraint (knot_point_constraint.jl:27-107) */
#define DTO_CONSTRAINT_NORM_MINUS_C 1   /* g(v) = [ ||v||_2   - c ] */
#define DTO_CONSTRAINT_SQNORM_MINUS_C 2 /* g(v) = [ ||v||_2^2 - c ] */
#define DTO_CONSTRAINT_QUADFORM_MINUS_C 5 /* g(v) = [ v' M v - c ], M symmetric n_comps x n_comps, passed in `hess0` (column-major,
                                           copied at create; M[a,b] == M[b,a] exactly, no component listed twice in `comps`).
                                           Expectation values, weighted populations, subspace fidelities; a final-fidelity
                                           bound ||A v||^2 >= F_min is M = -A'A, c = -F_min, equality = 0.  Evaluated on the
                                           device like the two kinds above (csrc/dto_quadform.hip): Jacobian entries 2 (M v)_c
                                           with the pattern of the numeric Jacobian at Z0, Hessian block 2 mu_i M (exact zeros of
                                           M are not added) */
#define DTO_CONSTRAINT_EXTERNAL_GLOBAL 4 /* NonlinearGlobalConstraint g(global_data[comps]) with g_dim outputs
                                           (global_constraint.jl:20-160): host closure; `comps` index global_data,
                                           `times` is unused; patterns = non-zeros of `jac0` (g_dim x n_comps) and
                                           of `hess0` (n_comps x n_comps, mu = ones; evaluator.jl:166) */
#define DTO_CONSTRAINT_EXTERNAL 3       /* host closure g with g_dim outputs: values, Jacobian blocks and
                                           mu-weighted Hessian blocks come from the caller (dto_set_external),
                                           evaluated with the reference's own code (knot_point_constraint.jl:
                                           235-294); the sparsity pattern is that of `jac0` */

typedef struct dto_integrator_desc {
    int32_t kind;
    int32_t x_off;  /* state component offset inside a knot (0-based) */
    int32_t x_dim;
    int32_t u_off;  /* bilinear: control offset; derivative: offset of the derivative component */
    int32_t u_dim;  /* bilinear: number of drives m; derivative: ignored (= x_dim) */
    const double* G; /* bilinear: (m+1) matrices x_dim*x_dim, column-major, G[0] = G(0) (drift),
                        G[j] = G(e_j) - G(0) (drive j); copied at create.  NULL for derivative. */
    /* DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR only (zero / NULL otherwise) */
    int32_t t_off;        /* component offset of the time variable t inside a knot (0-based) */
    int32_t spline_order; /* 0: controls held over the interval, 1: linearly interpolated to u_{k+1} */
    int32_t substeps;     /* fixed RK4 steps per interval */
    int32_t n_mod;        /* number of modulation terms c */
    const int32_t* mod_kind; /* [n_mod] 1 = cos(omega t), 2 = sin(omega t) */
    const double* mod_omega; /* [n_mod] */
    const double* H;         /* [n_mod][(m+1)] matrices x_dim*x_dim, column-major; copied at create */
} dto_integrator_desc;

typedef struct dto_objective_desc {
    int32_t kind;
    int32_t comp_off;
    int32_t comp_dim;
    int32_t reserved;
    double weight;          /* CompositeObjective weight (_objectives.jl:106-156) */
    double D;               /* MinimumTimeObjective scale */
    const double* R;        /* comp_dim weights (regularizers); LOWRANK_INFIDELITY: the factor A */
    const double* baseline; /* comp_dim x N column-major, or NULL = zeros (QuadraticRegularizer) */
    const int64_t* times;   /* 1-based knot indices, or NULL = 1:N */
    int64_t n_times;
    /* knot-point kinds (KNOT_SQDIST, KNOT_LOWRANK_INFIDELITY, EXTERNAL_KNOT): */
    const int32_t* comps;   /* knot-local component indices (0-based), vcat of var_names comps */
    int32_t n_comps;
    int32_t reserved2;
    const double* params;   /* n_comps x n_times column-major targets p_i, or NULL = zeros */
    const double* Qs;       /* n_times weights Q_i, or NULL = ones */
    const int32_t* gcomps;  /* EXTERNAL_GLOBAL: indices into global_data (0-based), vcat of global_names comps */
    int32_t n_gcomps;
    int32_t reserved3;
} dto_objective_desc;

typedef struct dto_constraint_desc {
    int32_t kind;
    int32_t equality;       /* 1: g = 0, 0: g <= 0 (src/solvers/solve.jl:54-62) */
    int32_t n_comps;
    int32_t g_dim;          /* outputs per listed time; 0 or 1 for the built-in kinds */
    const int32_t* comps;   /* knot-local component indices (0-based), vcat of var_names comps */
    double c;
    const int64_t* times;   /* 1-based knot indices (required) */
    int64_t n_times;
    const double* jac0;     /* EXTERNAL only: Jacobian blocks at Z0, [n_times] blocks g_dim x n_comps column-major;
                               entries that are exactly 0.0 are outside the pattern (evaluator.jl:136) */
    const double* hess0;    /* EXTERNAL_GLOBAL: Hessian of sum(g) at Z0, n_comps x n_comps column-major;
                               QUADFORM_MINUS_C: the matrix M, n_comps x n_comps column-major */
} dto_constraint_desc;

/* dto_problem_desc.flags */
#define DTO_FLAG_GENERAL_PATH_ONLY 1 /* bilinear integrators with <= 32 states also take the batched-GEMM path instead of
                                        the fused one-workgroup-per-interval kernel (tests run both and compare) */

#define DTO_FLAG_BLOCK_GENERATORS 2   /* look for replicated blocks in the generators of every DTO_INTEGRATOR_BILINEAR at create:
                                        the largest r dividing x_dim with G_j == I_r (x) B_j for all m+1 generators (exact
                                        comparison with ==).  Such an integrator -- an operator state in isomorphic coordinates,
                                        x = vec(X), X of b x r, b = x_dim / r -- is served by the structured path when r >= 2,
                                        b <= 64 and x_dim > 32: b x b work per interval instead of x_dim x x_dim, same value
                                        layout, same structure (dto_integrator_blocks tells).  The options that concern the dense
                                        chain and its sweeps (chain_form, chain_chunk, expm_form, sweep_form, reuse_forward_sweep,
                                        overlap_sweep) are accepted and have no effect on a structured integrator; its J w and
                                        J' w products go through the value slab.  The same search runs on every
                                        DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR over all (m+1)(1+n_mod) matrices G_j and H_cj (an
                                        all-zero matrix conforms): r >= 2, b <= 64, 32 < x_dim <= 512, state, controls, t and dt
                                        disjoint components, and the kind's substeps and coefficient-table limits put it on the
                                        structured time-dependent path (same discrete map on b x b); otherwise it is served as
                                        with the flag clear */

#define DTO_FLAG_SHARED_GENERATORS 4  /* look for DTO_INTEGRATOR_BILINEAR integrators that are driven by the same system: equal x_dim, the same
                                        control component (u_off, u_dim) and all m+1 generators equal entry by entry (==, no tolerance) --
                                        the kets of a multi-state transfer or ensemble problem, each with its own
                                        BilinearIntegrator(G, :psi_i, :u).  Their propagators exp(dt_k G(u_k)) are the same matrices: the
                                        first member in list order (the LEADER) runs the propagator chain of eval_constraint_jacobian, the
                                        others (FOLLOWERS) receive copies of its -E_k blocks (csrc/dto_share.hip) and run only their own
                                        tangent sweep, planned from the leader's norms.  A group is ACTIVE (shares) when it has two members
                                        or more and its members take the dense chain (33 states and up, or DTO_FLAG_GENERAL_PATH_ONLY);
                                        integrators on the small path or the structured path are reported as grouped but keep their
                                        evaluation.  Same structure, same value layout, the followers' blocks bit-identical to the leader's
                                        (dto_integrator_share tells).  eval_constraint, the Hessian and the matrix-free J w / J' w form
                                        no propagator and are not changed.
                                        DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR integrators are grouped among themselves (never with the
                                        bilinear kind): equal x_dim, the same control component (u_off, u_dim) and time component t_off,
                                        equal spline_order, substeps and n_mod, every modulation's kind and omega equal, and all
                                        (m+1)(1+n_mod) matrices G_j, H_cj equal entry by entry (==).  A group is ACTIVE when it has two
                                        members or more on the dense MFMA path (65..256 states, not on the structured path): one launch per
                                        group and callback (eval_constraint, Jacobian, Hessian) then forms every M0 = sum_q c_q B_q, every
                                        coefficient table and the Jacobian's Phi block once and carries each member's own vectors beside
                                        them (csrc/dto_tdb_mfma.hip, group form).  A member's values are bit-identical to the unflagged
                                        handle's.  A launch takes as many members as an 8 MiB scratch slot per resident workgroup admits
                                        (at most 8), larger groups run in consecutive launches; option "tdb_share_members" lowers the
                                        count.  Groups of 1..64 states or on the structured path are reported as grouped, inactive, and
                                        evaluated as with the flag clear; the matrix-free J w / J' w stay one launch per member */

typedef struct dto_problem_desc {
    int32_t abi_version;    /* DTO_ABI_VERSION */
    int32_t device;         /* HIP device ordinal */
    int64_t N;              /* knots */
    int32_t z;              /* traj.dim: components per knot */
    int32_t gd;             /* traj.global_dim */
    int32_t dt_idx;         /* component index of the timestep inside a knot (0-based); the engine
                               requires a timestep COMPONENT (bilinear_integrator.jl:123) */
    int32_t eval_hessian;   /* Evaluator(...; eval_hessian) -> features_available (evaluator.jl:293) */
    int32_t n_integrators;
    int32_t n_objectives;
    int32_t n_constraints;
    int32_t flags;          /* DTO_FLAG_* bits, 0 by default */
    const dto_integrator_desc* integrators;
    const dto_objective_desc* objectives;
    const dto_constraint_desc* constraints;
    const double* Z0;       /* initial point, length z*N+gd: constraint sparsity patterns are taken
                               from the numeric Jacobian at Z0 (evaluator.jl:136) */
    int64_t k_lo, k_hi;     /* owned knot range, 1-based inclusive; 0,0 = whole trajectory */
} dto_problem_desc;

typedef struct dto_handle dto_handle;

typedef struct dto_shard_info {
    int64_t k_lo, k_hi;
    int64_t n_vars, n_cons, jac_nnz, hess_nnz;     /* GLOBAL sizes */
    int64_t grad_lo, grad_len;                      /* gradient slab: entries of owned knots */
    int64_t jac_lo, jac_len;                        /* Jacobian value slab (CSC order)        */
    int64_t hess_lo, hess_len;                      /* Hessian value slab (upper-tri CSC order) */
    int64_t cons_len;                               /* local constraint rows (see dto_shard_rows) */
    int32_t n_row_segments;
    int32_t reserved;
} dto_shard_info;

/* lifecycle -- replaces Evaluator(prob; eval_hessian) at ipopt_solver/solver.jl:68-69 and
 * ext/MadNLPSolverExt/solver.jl:81 */
int dto_create(const dto_problem_desc* desc, dto_handle** out);
void dto_destroy(dto_handle* h);
const char* dto_last_error(const dto_handle* h); /* h may be NULL: error of the last failed create */

/* sizes: Evaluator fields n_constraints / n_dynamics_constraints / n_nonlinear_constraints
 * (evaluator.jl:73-76) and structure lengths */
int dto_num_vars(const dto_handle* h, int64_t* out);
int dto_num_cons(const dto_handle* h, int64_t* out);
int dto_num_dynamics_cons(const dto_handle* h, int64_t* out);
int dto_jac_nnz(const dto_handle* h, int64_t* out);
int dto_hess_nnz(const dto_handle* h, int64_t* out);
int dto_features_available(const dto_handle* h, int32_t* grad, int32_t* jac, int32_t* hess); /* evaluator.jl:293-299 */
int dto_get_shard_info(const dto_handle* h, dto_shard_info* out);
/* local constraint buffer = concatenation of global row segments [start1 (1-based), len] */
int dto_shard_rows(const dto_handle* h, int64_t* start1, int64_t* len);

/* finest replicated-block structure found in integrator i (0-based) and whether the structured path serves it;
   (x_dim, 1, 0) when the flag is clear, the kind is neither bilinear nor time-dependent bilinear, or no structure exists */
int dto_integrator_blocks(const dto_handle* h, int32_t integrator, int32_t* block_dim, int32_t* reps, int32_t* active);

/* the group of integrator i (0-based) under DTO_FLAG_SHARED_GENERATORS: its leader (0-based position in the integrator list), the
   number of members, and whether the group shares -- one propagator chain (bilinear), one propagation per callback
   (time-dependent bilinear); (i, 1, 0) when the flag is clear, the kind is neither bilinear nor time-dependent bilinear, or the
   integrator has no partner */
int dto_integrator_share(const dto_handle* h, int32_t integrator, int32_t* leader, int32_t* group_size, int32_t* active);

/* Cost model of one eval_constraint_jacobian for intervals first .. first+count-1 (0-based, GLOBAL numbering; Z is the whole NLP
 * vector, host memory): flops from the growth bound of every interval's A_k = dt_k G(u_k) -- squarings of the propagator chain,
 * Taylor terms of the sweep (bilinear_integrator.jl:81: `expv`'s work grows with ||dt G(u)|| too).  Host arithmetic only, also on
 * structure-only handles: a caller that shards knot ranges over GPUs balances them by these instead of by knot
 * count, so that on a pulse whose amplitude varies along the trajectory the slowest rank does not set the step; unequal ranges
 * are gathered in the broadcast form (dto_get_gather_layout). */
int dto_interval_costs(const dto_handle* h, const double* Z, int64_t first, int64_t count, double* cost);

/* structure -- MOI.jacobian_structure (evaluator.jl:364) / MOI.hessian_lagrangian_structure (:385).
 * Writes entries [first, first+count) (0-based position in the GLOBAL CSC order), 1-based pairs. */
int dto_jacobian_structure(const dto_handle* h, int64_t first, int64_t count, int64_t* rows, int64_t* cols);
int dto_hessian_structure(const dto_handle* h, int64_t first, int64_t count, int64_t* rows, int64_t* cols);
/* row bounds handed to the solver, src/solvers/solve.jl:30-65: lower/upper per NLP row */
int dto_constraint_bounds(const dto_handle* h, double* lower, double* upper);

/* Host-evaluated ("external") terms -- SURVEY.md §8f rank 2.  One entry per EXTERNAL term: the external
 * integrators in list order, then the external constraints in list order, then the external objectives.  All pointers are HOST
 * pointers; they are read (copied to the device) by every callback that follows until replaced, so the shim
 * fills whatever the next callback needs and calls dto_set_external first.  Arrays cover ALL listed times of the
 * term, in list order; a sharded handle reads only the blocks of its own knots.
 *   integrator: values = defects, [N-1] x x_dim;  first = Jacobian blocks, [N-1] x (x_dim x 2z col-major, columns
 *               z_k then z_{k+1});  second = Hessian blocks of mu_k' f, [N-1] x (2z x 2z col-major) -- accumulated (+=)
 *               like every integrator block (evaluator.jl:574-598), row <= col entries only
 *   constraint: values = g, [n_times] x g_dim;  first = Jacobian blocks, [n_times] x (g_dim x n_comps col-major);
 *               second = Hessian blocks of mu_i' g, [n_times] x (n_comps x n_comps col-major)
 *   global constraint: values = g [g_dim]; first = Jacobian g_dim x n_comps col-major; second = Hessian of mu' g
 *   global objective:  as "objective" below with v_i = [z_t[comps]; global_data[gcomps]] (block size n_comps + n_gcomps)
 *   objective:  values = Q_i l(v_i, p_i), [n_times];  first = Q_i grad l, [n_times] x n_comps;
 *               second = Q_i Hessian of l, [n_times] x (n_comps x n_comps col-major)
 * Semantics follow the reference: Jacobian entries are assigned, outside-pattern entries dropped
 * (evaluator.jl:491-551); gradient!/hessian! overwrite per listed time, so for a knot listed twice the later
 * block wins; only row <= col Hessian entries are kept (evaluator.jl:637). */
typedef struct dto_external_values {
    const double* values;
    const double* first;
    const double* second;
} dto_external_values;
int dto_num_external(const dto_handle* h, int32_t* n_integrators, int32_t* n_constraints, int32_t* n_objectives);
int dto_set_external(dto_handle* h, int32_t n, const dto_external_values* v);

/* host-pointer callbacks (blocking) */
int dto_eval_objective(dto_handle* h, const double* Z, double* f);                 /* evaluator.jl:304 */
int dto_eval_gradient(dto_handle* h, const double* Z, double* grad);               /* evaluator.jl:310 */
int dto_eval_constraint(dto_handle* h, const double* Z, double* g);                /* evaluator.jl:323 */
int dto_eval_jacobian(dto_handle* h, const double* Z, double* vals);               /* evaluator.jl:368 */
int dto_eval_hessian(dto_handle* h, const double* Z, double sigma, const double* mu,
                     double* vals);                                                /* evaluator.jl:389 */
/* y = J w  /  y = J' w without materialising J on the host (evaluator.jl:406-456).  Unsharded handles only.  y is written in
   full.  Handles made of bilinear integrators (structured, small or general), DerivativeIntegrators and built-in knot constraints
   form no Jacobian at all: each integrator contracts its sweep with w and the handle never holds a jac_len-sized
   allocation for the products.  Handles with a time-dependent integrator (unless option "tdb_matrix_free_products" is 1, which
   serves every device path of theirs, the structured one of DTO_FLAG_BLOCK_GENERATORS included) or an external integrator, an
   external constraint, more than MAX_TYPES - 2 drives, or (J' w only) a general-path integrator created with eval_hessian = 0
   evaluate the Jacobian into a private device slab, allocated at the first product, and contract that.  The `_dev` forms below run the same device routine on
   the caller's pointers and stream: both families return the same bits. */
int dto_eval_jacobian_product(dto_handle* h, const double* Z, const double* w, double* y);
int dto_eval_jacobian_transpose_product(dto_handle* h, const double* Z, const double* w, double* y);
/* y = H(Z; sigma, mu) v, H the symmetric matrix whose upper triangle is dto_hessian_structure / dto_eval_hessian
   (off-diagonal entries count for (i,j) and (j,i), as MOI defines it); MOI.eval_hessian_lagrangian_product.
   y [n_vars] is written in full (0 where H has no entry); H is exactly what dto_eval_hessian returns at that point.
   Unsharded handles created with eval_hessian = 1 only (an error with text otherwise).  The engine assembles H once per
   point into a private device slab and keeps a compact row-major copy of both triangles; a product at the same
   (Z, sigma, mu) -- bit for bit, with no dto_set_external, dto_set_option or failed call since -- is one launch.  The copy
   costs the handle a second Hessian slab plus 20 bytes per stored entry (about 2 x 1 % of the slab). */
int dto_eval_hessian_product(dto_handle* h, const double* Z, double sigma, const double* mu,
                             const double* v, double* y);

/* device-pointer callbacks (asynchronous on `stream`; outputs stay in HBM) */
int dto_eval_objective_dev(dto_handle* h, const double* dZ, double* df, void* stream);
int dto_eval_gradient_dev(dto_handle* h, const double* dZ, double* dgrad, void* stream);
int dto_eval_constraint_dev(dto_handle* h, const double* dZ, double* dg, void* stream);
int dto_eval_jacobian_dev(dto_handle* h, const double* dZ, double* dvals, void* stream);
int dto_eval_hessian_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu,
                         double* dvals, void* stream);
/* the same product on device pointers; waits on one 4-byte readback when the handle holds a cached point */
int dto_eval_hessian_product_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu,
                                 const double* dv, double* dy, void* stream);
/* y = J w (dw [n_vars], dy [n_cons]) and y = J' w (dw [n_cons], dy [n_vars]) on device pointers: enqueued on `stream`, nothing
   crosses the bus, errors are deferred as for every `_dev` call, one call in flight per handle */
int dto_eval_jacobian_product_dev(dto_handle* h, const double* dZ, const double* dw, double* dy, void* stream);
int dto_eval_jacobian_transpose_product_dev(dto_handle* h, const double* dZ, const double* dw, double* dy, void* stream);

/* ---- Open-loop rollout: X_{k+1} = E_k(Z) X_k, k = 1 .. N-1, X_1 = X0 -- the states an integrator's dynamics reach from X0 under the
 * controls, timesteps and (time-dependent kind) times of Z, whatever states Z itself holds.  This is what the reference's rollout
 * callbacks evaluate every few iterations (callback_rollout_fidelity_factory / callback_best_rollout_fidelity_factory,
 * src/solvers/ipopt_solver/callbacks.jl:264-361: `fid_fn(problem.trajectory, system)`): while the dynamics constraints are still
 * violated, the fidelity of the ROLLED-OUT final state tells more than the objective does.
 *   E_k is the propagator of interval k of integrator `integrator` (0-based position in the integrator list) at Z: exactly the
 *   matrix whose negative dto_eval_jacobian stores in that integrator's x_k columns -- exp(dt_k G(u_k)) for DTO_INTEGRATOR_BILINEAR on
 *   every path (small, 33..64 states, general, structured, leader or follower of a shared group), the RK4 map Phi_k for
 *   DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR on every device path.  The state components of Z are not read, unless X0 is NULL.
 *   X0: x_dim x n_cols column-major, 1 <= n_cols <= x_dim (a full basis gives the cumulative propagators: the unitary rollout);
 *   NULL takes the integrator's state components of knot 1 of Z and requires n_cols = 1.
 *   X:  DTO_ROLLOUT_ALL   [N][n_cols][x_dim] -- knot-major, then column, rows contiguous; knot 1 is a copy of X0
 *       DTO_ROLLOUT_FINAL [n_cols][x_dim], the states at knot N: bit for bit the last block of DTO_ROLLOUT_ALL
 * The call evaluates the Jacobian at Z into a private device slab (shared with the slab route of the Jacobian-vector products),
 * gathers the N-1 blocks into a balanced binary tree of batched FP64 matrix products (ceil(log2(N-1)) launches) and descends the tree
 * with one launch per level.  Every entry of X has one writer and a fixed summation order: a column has the same bits alone and
 * among others, repeated calls are bit-identical, and both entry-point families return the same bits.  Workspaces are allocated at
 * the first rollout, grow only and are freed with the handle: the tree, (2^(L+1) - 1) npad^2 doubles with 2^L >= N-1 and npad =
 * x_dim rounded up to 64, a padded trajectory of N x n_cols (rounded up to 16; to 64 from 49 on) x npad doubles, and the Jacobian slab.
 * Refused with text, the handle stays usable: a DerivativeIntegrator or external integrator, an index out of range, a sharded handle,
 * a structure-only handle, n_cols out of range, a mode other than the two, a failed workspace allocation.
 * The `_dev` form works on the caller's stream with outputs in HBM, may wait on the same small readbacks as dto_eval_jacobian_dev,
 * and defers device-side errors as every `_dev` call; the host-pointer form uploads, runs the same device routine, downloads and blocks. */
#define DTO_ROLLOUT_ALL 0
#define DTO_ROLLOUT_FINAL 1
int dto_rollout(dto_handle* h, int32_t integrator, const double* Z, const double* X0, int32_t n_cols, int32_t mode, double* X);
int dto_rollout_dev(dto_handle* h, int32_t integrator, const double* dZ, const double* dX0, int32_t n_cols, int32_t mode,
                    double* dX, void* stream);

/* ---- Solves with the dynamics block: linearised and adjoint rollouts.  M is the block of the Jacobian formed by integrator
 * `integrator`'s rows and its own state columns, with the identity row of knot 1 on top: I on the diagonal, -E_k(Z) below it (E_k as
 * for dto_rollout above; the state components of Z are not read).
 *   DTO_SOLVE_FORWARD  M Y = B:    Y_1 = B_1,  Y_{k+1} = E_k Y_k + B_{k+1} -- the linearised rollout.  B = -(defect of Z) gives the
 *                      state correction that makes a trajectory dynamically feasible under its controls; B = [X0; 0; ...] is
 *                      dto_rollout, bit for bit.
 *   DTO_SOLVE_ADJOINT  M' Lam = B: Lam_N = B_N,  Lam_k = E_k' Lam_{k+1} + B_k -- the costate recursion.  With B the gradient of a loss of
 *                      the rolled-out states and w holding Lam_2 .. Lam_N in the integrator's rows, -J' w (dto_eval_jacobian_transpose_
 *                      product) is the gradient of that loss with respect to the controls and timesteps.
 *   B, Y: [N][n_cols][x_dim] in the layout of dto_rollout's X, 1 <= n_cols <= x_dim; they must not overlap.  `mode` is dto_rollout's:
 *   DTO_ROLLOUT_FINAL returns [n_cols][x_dim], the block at knot N (forward) or at knot 1 (adjoint), bit for bit that block of
 *   DTO_ROLLOUT_ALL.  N = 1 returns B.
 * Both solves are affine scans over dto_rollout's product tree: an offset block per node, one launch per level up and one per level
 * down, the adjoint through a transposed left operand (no second tree).  Every entry has one writer and a fixed summation order: a
 * column has the same bits alone and among others, repeated calls are bit-identical, both entry-point families return the same bits.
 * The tree is kept per point: a solve at the Z of the last one -- bit for bit, the same integrator, with no dto_set_external,
 * dto_set_option, failed call or dto_rollout since -- runs its scan alone, after one device-side compare with a 4-byte readback;
 * otherwise the call evaluates the Jacobian into the private slab and rebuilds the tree as dto_rollout does.  Workspaces beside
 * dto_rollout's (shared with it), grow-only, freed with the handle: the offset tree, (2^(L+1) - 1) x n_cols (padded as the trajectory)
 * x npad doubles, and a copy of Z.
 * Refused with text, the handle stays usable: everything dto_rollout refuses, a direction other than the two, B = NULL.
 * The `_dev` form works on the caller's stream and defers device-side errors as every `_dev` call; solves at one point enqueued on
 * different streams are the caller's to order. */
#define DTO_SOLVE_FORWARD 0
#define DTO_SOLVE_ADJOINT 1
int dto_dynamics_solve(dto_handle* h, int32_t integrator, const double* Z, int32_t direction, const double* B, int32_t n_cols, int32_t mode,
                       double* Y);
int dto_dynamics_solve_dev(dto_handle* h, int32_t integrator, const double* dZ, int32_t direction, const double* dB, int32_t n_cols,
                           int32_t mode, double* dY, void* stream);

/* ---- Whole-dynamics solves: all integrators' states at once.  With I integrators of state components S_i = [x_off, x_off + x_dim),
 * D = sum x_dim and pre_i the sum of the dimensions before i in list order, MM is the N D x N D block of the Jacobian formed by ALL
 * integrators' rows and ALL their state columns: per integrator an identity row block for knot 1, below it its defect rows of
 * intervals 1 .. N-1 restricted to the columns S_j of every knot -- entry for entry what dto_eval_jacobian returns at Z.  Besides the
 * diagonal blocks M_i of dto_dynamics_solve it holds the couplings: the controls of a bilinear integrator that a DerivativeIntegrator
 * integrates, du / ddu chains, a time-dependent integrator of spline order 1 reaching u_{k+1}.
 *   DTO_SOLVE_FORWARD  MM Y = B.  B = -(defect of Z) with zero knot-1 rows gives the first-order state correction of the whole
 *                      trajectory under fixed controls.
 *   DTO_SOLVE_ADJOINT  MM' Lam = B: the costates of all dynamics rows; Lam_1 is the derivative with respect to the initial states.
 *   B, Y: [N][n_cols][D], the D axis listing the integrators in list order, x_dim contiguous each (dto_dynamics_layout); they must
 *   not overlap.  1 <= n_cols <= the smallest x_dim among the bilinear and time-dependent integrators (each block solve's own limit);
 *   1 .. 64 on a handle with DerivativeIntegrators only.  All knots are returned.
 * MM is block-triangular in DEPENDENCY order: integrator a depends on b != a when S_b meets a's inputs -- the controls and the
 * timestep component (bilinear), these and the time component (time-dependent), the derivative's components and the timestep
 * component (derivative).  level(a) = 0 without dependencies, else 1 + max level(deps).  The forward solve visits the integrators by
 * (level, list position) ascending: B'_{k+1} = B_{k+1} - C_{a,k} [Y^deps_k ; Y^deps_{k+1}], then a's own block solve; the adjoint solve
 * in the reverse order with B'_k = B_k - sum over a's dependents b of C_b' Lam^b (dependents in list order, interval k-1 before k, rows
 * ascending).  Every entry has one writer and a fixed summation order, without atomics: repeated calls are bit-identical, both
 * entry-point families return the same bits, a column has the same bits alone and among others, a rebuilt point gives the bits of a
 * cached one.  The block of a level-0 DerivativeIntegrator is the serial sum Y_{k+1} = Y_k + B_{k+1} (Lam_k = Lam_{k+1} + B_k) in
 * double, bit for bit.
 * At a new point the call evaluates the Jacobian ONCE into the private slab, builds a product tree per bilinear and time-dependent
 * integrator, copies the coupling blocks into a compact store and keeps a copy of Z.  These are the call's own workspaces -- one tree
 * of (2^(L+1) - 1) npad^2 doubles PER integrator (members of a shared-generator group included), the store of
 * (N-1) x 2 x x_dim_a x (sum of its dependencies' x_dim) doubles per integrator a -- grow-only, freed with the handle; dto_rollout and
 * dto_dynamics_solve neither read nor disturb them.  They are kept per point as dto_dynamics_solve keeps its tree: a call at the Z of
 * the last one, bit for bit, with no dto_set_external, dto_set_option or failed call since, launches no Jacobian, gather or tree kernel.
 * Refused with text, the handle stays usable: a host-evaluated integrator anywhere in the handle, a sharded or structure-only handle,
 * integrators whose states overlap, an integrator whose inputs meet its own states, a dependency cycle, n_cols out of range, a
 * direction other than the two, B = NULL, a failed workspace allocation.
 * dto_dynamics_layout: D, the number of levels, and per integrator its offset pre_i on the D axis and its level (either array may be
 * NULL); it needs no device and answers on structure-only handles too. */
int dto_dynamics_layout(const dto_handle* h, int32_t* n_states, int32_t* n_levels, int32_t* offset /*[n_integrators]*/, int32_t* level /*[n_integrators]*/);
int dto_dynamics_solve_all(dto_handle* h, const double* Z, int32_t direction, const double* B, int32_t n_cols, double* Y);
int dto_dynamics_solve_all_dev(dto_handle* h, const double* dZ, int32_t direction, const double* dB, int32_t n_cols, double* dY, void* stream);

/* ---- Reduced-space operators: the gradient and the Hessian-vector product of the problem with the states eliminated by the dynamics
 * -- the control-only view a GRAPE-style or truncated-Newton method works in.  S is the set of DEPENDENT entries of Z: the state
 * components [x_off, x_off + x_dim) of every integrator at knots 2 .. N; C is every other entry (controls, timesteps, times, the states
 * of knot 1, globals).  MM, D, pre_i and the [N][n_cols][D] layout are those of dto_dynamics_solve_all; the dynamics rows of integrator
 * i start at its row offset, interval k (0-based) taking x_dim rows from row0_i + k x_dim.  With sigma and mu (length n_cons, or NULL
 * for zeros; its dynamics-row entries are never read),  phi(Z) = sigma f(Z) + sum over the non-dynamics rows r of mu_r g_r(Z).
 *   dto_reduced_gradient   g = sigma grad f(Z) + J' w1, w1 = mu with its dynamics rows set to 0 (mu = NULL: the product is skipped);
 *                          MM' Lam = g_S, g_S the state entries of g at all knots as [N][1][D];  t = J' w2, w2 zero except
 *                          Lam_2 .. Lam_N in the dynamics rows.  grad [n_vars]: g - t on C except the states of knot 1, Lam_1 on the
 *                          states of knot 1, 0 on S.  lam (may be NULL): Lam as [N][D], the costates.
 *   dto_reduced_hessian_product   y = T' H(Z; sigma, mu~) T v, T the tangent map of the feasible manifold (identity on C,
 *                          -J_S^-1 J_C on S) and mu~ = mu on the non-dynamics rows, -Lam_{k+1} on the dynamics rows of interval k:
 *                            1. v^ = v with the state entries of ALL knots zeroed, rho = J v^          (the S entries of v are not read)
 *                            2. B_1 = the knot-1 state entries of v, B_{k+1} = -rho[dynamics rows of interval k]
 *                            3. MM Y = B                     4. z^ = v^ with the state entries of all knots set to Y
 *                            5. q = H(Z; sigma, mu~) z^      6. MM' Gam = q_S
 *                            7. t = J' w, w zero except Gam_2 .. Gam_N in the dynamics rows
 *                            8. y = q - t on C except the states of knot 1, Gam_1 on the states of knot 1, 0 on S.
 *                          v, y [n_vars]; they must not overlap.
 * At a dynamically feasible Z the gradient is that of phi(feasible trajectory(.)) and the product its Hessian; at any other Z they are
 * the reduced gradient and Hessian of an SQP method.  The product is symmetric either way.
 * The arithmetic outside the engine's own routines is sigma * (.), one addition, one subtraction and negations, each rounded on its
 * own: the results are, bit for bit, those of the same steps written with dto_eval_gradient, dto_eval_jacobian_product,
 * dto_eval_jacobian_transpose_product, dto_dynamics_solve_all (one column) and dto_eval_hessian_product and repacked on the host.
 * Repeated calls, both entry-point families and a rebuilt point against a kept one return the same bits.
 * Cache rule.  The REDUCED POINT -- g, Lam, mu~ and the reduced gradient -- is kept per (Z, sigma, mu): Z and mu bit for bit (mu = NULL
 * is a point of its own), with no dto_set_external, dto_set_option or failed call since; one device-side compare with a 4-byte
 * readback decides.  The kept copies are written on the stream of the call that computed them and compared on the stream of the next
 * call, as for the per-point caches of the routines inside: use ONE stream at a time per handle, or order the streams yourself
 * (an event, a synchronize) before a call on another one.  A gradient at the kept point copies its results; a product at a new point first computes the gradient's
 * quantities; a product at the kept point runs steps 1 .. 8 alone.  The routines inside keep their own per-point caches and their own
 * 4-byte readbacks (three per product at the kept point: two solves, one H v): both solves reuse the trees from the first product on,
 * and since mu~ is then bit-identical the Hessian is assembled for the first product only -- until a dto_eval_hessian_product at
 * another (Z, sigma, mu) takes its slab, which costs the next reduced product one re-assembly and changes no bit.
 * Costs at the kept point: one J w, one J' w, two whole-dynamics scans, one H v and six packer launches (O(n_vars + n_cons + N D)
 * bytes each); no Jacobian chain, tree build or Hessian assembly -- EXCEPT on handles whose J w / J' w take the slab route (a
 * time-dependent integrator without the option "tdb_matrix_free_products", more than MAX types of drives, ...): there each of the two
 * products evaluates the Jacobian.  At a new point add: the objective gradient, one or two J' w, the Jacobian with the trees and the
 * coupling store (dto_dynamics_solve_all), one adjoint scan, the Hessian assembly.
 * Workspaces: one block of 7 n_vars + 4 n_cons + 3 N D doubles, allocated at the first call before anything is enqueued and freed
 * with the handle, besides those of the routines inside.
 * Option "reduced_input_store" (default 0; dto_set_option, values other than 0 and 1 are refused): 1 takes rho = J v^ (steps 1 - 2) and
 * t = J' w (steps 7 - 8, and t = J' w2 of the gradient) from a kept INPUT-BLOCK STORE instead of dto_eval_jacobian_product /
 * _transpose_product.  In step 1 only the non-state entries of v^ are non-zero and only the dynamics rows of rho are read; in step 7 w
 * is zero outside the dynamics rows and only the non-state entries of t are read: both are products with the block
 * J[dynamics rows, non-state knot components].  A FREE INPUT of integrator a is a component it reads (its controls or the derivative's
 * components, the timestep, for time-dependent integrators the time) that is no integrator's state; fin_a lists them ascending, Wf_a
 * is their number.  The store F_a [N - 1][2][Wf_a][x_dim_a] holds a's rows of interval k in the columns fin_a of knot k (half 0) and
 * knot k + 1 (half 1; non-zero for spline order 1 only), rows contiguous, the integrators' stores one behind the other in list order:
 * the sum over a of (N - 1) 2 Wf_a x_dim_a doubles, grow-only, allocated before anything is enqueued.  It is gathered from the private
 * Jacobian slab in the rebuild of dto_dynamics_solve_all's point, beside the coupling blocks, and kept with that point.
 * Summation orders (every product and sum rounded on its own, never contracted).  B_1 = the knot-1 state entries of v; for k >= 1, a
 * the owner of D position d and r = d - pre_a:  acc = 0, then half 0 before half 1 and j ascending inside each,
 * acc += F_a[k-1][half][j][r] v[(k - 1 + half) z + fin_a[j]], and B_{k+1}[d] = -acc.  y: 0 on S, Gam_1 on the states of knot 1, q - 0.0
 * on globals and on knot components no integrator reads, q - t on a free-input component c of knot kn (0-based), t summed by one
 * wavefront: lane l adds, over c's readers (a, j) in list order, per reader interval kn - 1 through half 1 (kn >= 1) and then interval
 * kn through half 0 (kn < N - 1), the rows r = l, l + 64, .. ascending, F_a[iv][half][j][r] Gam_{iv+2}[pre_a + r]; the 64 partial sums
 * are then combined by a fixed halving tree, p_l += p_{l+32}, p_l += p_{l+16}, .. , p_l += p_{l+1}, and t = p_0.  No atomics.
 * Results of the two routes agree to rounding (other summation orders); with 1 the bits are those of the sums above over the entries
 * of dto_eval_jacobian's values.  Repeated calls, both entry-point families and a rebuilt point return the same bits on either route.
 * Costs with 1, at the kept point: two products with the store (its bytes twice), two whole-dynamics scans, one H v and two packer
 * launches -- no J w, no J' w, on slab-route handles no Jacobian evaluation; the solves' point is checked once per product (two 4-byte
 * readbacks instead of three).  At a new point the gradient loses its second J' w and gains the gather.  The reduced point and the
 * solves' point are kept apart, so a dto_dynamics_solve_all at another Z between two products leaves the store stale: a product
 * first makes the solves' point its own Z -- after such a call one rebuild with ONE Jacobian evaluation -- and reads the store after that.
 * J' w1 of the constraint rows (mu given) stays dto_eval_jacobian_transpose_product.  With 0 nothing changes.
 * Refused with text, the handle stays usable and nothing is enqueued: everything dto_dynamics_solve_all refuses (a host-evaluated
 * integrator, a sharded or structure-only handle, overlapping states, an integrator reading its own states, a dependency cycle); any
 * host-evaluated constraint or objective; a handle without integrators; Z, grad, v or y = NULL; for the product a handle created
 * with eval_hessian = 0 (the gradient still works there).  The _dev forms take device pointers (dmu and dlam may be NULL), enqueue on
 * `stream` and defer device-side errors like every _dev call. */
int dto_reduced_gradient(dto_handle* h, const double* Z, double sigma, const double* mu, double* grad, double* lam);
int dto_reduced_gradient_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, double* dgrad, double* dlam, void* stream);
int dto_reduced_hessian_product(dto_handle* h, const double* Z, double sigma, const double* mu, const double* v, double* y);
int dto_reduced_hessian_product_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* dv, double* dy, void* stream);

/* ---- Block products: H V and T' H T V for n_cols vectors per call.  A block-Krylov method, a randomised preconditioner, several
 * Hessian probes or the explicit reduced Hessian of a small control space ask for many products at ONE point; the single products
 * read the Hessian copy, the solves' node matrices and the input blocks once per vector, these read them once per tile or chunk.
 *   dto_eval_hessian_products        column c of Y is H(Z; sigma, mu) V_c            (dto_eval_hessian_product for every column)
 *   dto_projected_hessian_products   column c of Y is T' H(Z; sigma, mu~) T V_c      (dto_reduced_hessian_product for every column)
 * Layout.  V and Y are [n_cols][n_vars]: column c contiguous at offset c n_vars.  They must not overlap.  n_cols >= 1, no upper limit.
 * Bit contract.  Column c of Y is, bit for bit, what the single product returns for V_c on the same handle -- for the projected
 * product with the same "reduced_input_store" setting.  Per column every kernel runs the single form's operations in the single form's
 * order (the H product: a lane's pairs l, l + G, .. then the butterfly; the input-block products: the orders stated above), and the
 * whole-dynamics solves return a column's bits alone or among others.  The results do not depend on n_cols, on the chunk width, on
 * the entry-point family, or on whether the point was kept or rebuilt.  The S entries of V are not read (a NaN there reaches nothing);
 * Y is 0 on S.
 * Chunking.  The engine works through the columns in chunks of W = min(cap, width): cap is dto_dynamics_solve_all's limit on n_cols
 * (the smallest x_dim among the integrators with a propagator, 64 without one; it does not apply to dto_eval_hessian_products), width
 * the option "reduced_block_width" (1 .. 64) or, with its default 0, the engine's choice (64).  Inside a chunk the H product and the
 * transposed input-block product hold tiles of 1, 2, 4 or 8 columns in registers.
 * Points.  dto_eval_hessian_products uses dto_eval_hessian_product's kept point: ONE point check per call, at the kept point no
 * assembly and one launch per chunk.  dto_projected_hessian_products uses the reduced point, the solves' point and the Hessian point
 * under the cache rule above, each checked ONCE per call (three 4-byte readbacks per call, not per chunk or column); a block call
 * after a single product at the same point, or the other way round, computes no new point.
 * Costs per chunk at the kept point, "reduced_input_store" = 1: two products with the store (its bytes twice), two whole-dynamics scans
 * of w columns, one block H product and two packer launches -- the launches of ONE single product; no Jacobian evaluation.  With 0 the
 * six packers run in block form and J v^ and J' w stay dto_eval_jacobian_product / _transpose_product, called once per column: on
 * handles whose products take the slab route this evaluates the Jacobian 2 n_cols times per call -- use the store route there.
 * Workspaces, grow-only and allocated before anything is enqueued: one block of W (2 n_vars + 2 N D) doubles (W n_cons more with
 * "reduced_input_store" = 0), what dto_dynamics_solve_all grows for n_cols = W, and for the host-pointer forms 2 n_cols n_vars doubles.
 * The single products' block and entry points are untouched.
 * Refused with text, the handle stays usable and nothing is enqueued: what the single product refuses; n_cols < 1; V or Y = NULL; a
 * failed workspace allocation.  The host-pointer forms upload V, run the device routine on the handle's stream, download Y and block;
 * both families return the same bits.  The _dev forms take device pointers, enqueue on `stream` and defer device-side errors like
 * every _dev call. */
int dto_eval_hessian_products(dto_handle* h, const double* Z, double sigma, const double* mu, int32_t n_cols, const double* V, double* Y);
int dto_eval_hessian_products_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, int32_t n_cols, const double* dV, double* dY, void* stream);
int dto_projected_hessian_products(dto_handle* h, const double* Z, double sigma, const double* mu, int32_t n_cols, const double* V, double* Y);
int dto_projected_hessian_products_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, int32_t n_cols, const double* dV, double* dY, void* stream);

/* ---- Feasible trajectory and merit value: the function the operators above are derivatives of, phi(feasible trajectory(Z)) -- what a
 * truncated-Newton or GRAPE-style method evaluates once per line-search trial, without leaving the device.
 *   dto_feasible_trajectory   Zf [n_vars] = Z with every integrator's state components at knots 2 .. N replaced by what its dynamics
 *                          reach from the knot-1 states under the controls, timesteps and times of Z.  Levels (dto_dynamics_layout)
 *                          run ascending.  Inside a level: first the DerivativeIntegrators in list order, each the recurrence
 *                          x_{k+1} = x_k + dt_k xdot_k with the product and the sum rounded on their own; then, if the level holds an
 *                          integrator with a propagator, ONE Jacobian evaluation at the Zf built so far into the private slab; then per
 *                          such integrator in list order its product tree from that slab (dto_rollout's), the descent through all knots
 *                          from the knot-1 state of Zf, and the scatter into Zf.  E_k reads no state of its own level, so one evaluation
 *                          serves every integrator of the level: one for a multi-ket problem, not one per ket.
 *                          Zf may equal Z (the _dev form then works in place); otherwise they must not overlap.  N = 1 returns a copy.
 *   dto_feasible_merit     runs the routine above, then the engine's own objective and constraint evaluation at Zf -- f and g have
 *                          the bits of dto_eval_objective_dev / dto_eval_constraint_dev there -- and
 *                              phi = sigma f + sum over the non-dynamics rows r of mu_r g_r(Zf)
 *                          summed by one wavefront in a fixed order: lane l adds mu_r g_r over r = n_dyn + l, n_dyn + l + 64, ..
 *                          ascending, every product and every sum rounded on its own; the 64 partial sums are combined by the halving
 *                          tree stated for the input-block product above (p_l += p_{l+32}, .. , p_l += p_{l+1}), t = p_0;
 *                          phi = sigma * f + t, product and sum rounded on their own.  mu = NULL: phi = sigma * f.  No atomics; the
 *                          dynamics-row entries of mu are never read.
 *                          phi: one double.  Zf [n_vars] may be NULL (the engine then works in a buffer of its own).  g may be NULL,
 *                          else [n_cons]: all rows at Zf -- the dynamics rows are the residual defects, which tell how feasible the
 *                          rollout is.  Without g and without mu the constraints are not evaluated.
 * Bits.  A DerivativeIntegrator's states are those of the recurrence written in NumPy; an integrator's rolled-out states are those of
 * dto_rollout (X0 = NULL) at the Z updated so far, whichever integrators share its level.  Repeated calls and both entry-point
 * families return the same bits.
 * Kept points.  The calls reuse dto_rollout's tree and trajectory workspaces and the private slab: like dto_rollout they drop the kept
 * point of dto_dynamics_solve.  The whole-dynamics solves' point, the reduced point and the Hessian products' point are not touched: a
 * line search between two reduced products costs those products nothing.
 * Workspaces, grow-only and allocated before anything is enqueued: dto_rollout's for the widest integrator with a propagator (one
 * column) and the private slab; for the merit one block of n_vars + 2 n_cons + 2 doubles.
 * Refused with text, the handle stays usable and nothing is written: everything dto_dynamics_solve_all refuses (a host-evaluated
 * integrator, a sharded or structure-only handle, overlapping states, an integrator reading its own states, a dependency cycle); Z or
 * Zf = NULL (the merit: Z or phi = NULL); for the merit any host-evaluated constraint or objective.
 * The host-pointer forms upload Z, run the device routine on the handle's stream, download and block.  The _dev forms take device
 * pointers (dmu, dZf and dg may be NULL), enqueue on `stream`, may wait on the small readbacks dto_eval_jacobian_dev waits on, and
 * defer device-side errors like every _dev call. */
int dto_feasible_trajectory(dto_handle* h, const double* Z, double* Zf);
int dto_feasible_trajectory_dev(dto_handle* h, const double* dZ, double* dZf, void* stream);
int dto_feasible_merit(dto_handle* h, const double* Z, double sigma, const double* mu, double* phi, double* Zf, double* g);
int dto_feasible_merit_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, double* dphi, double* dZf, double* dg, void* stream);

/* ---- Truncated-Newton step: the inner solve of a truncated-Newton or trust-region method on the reduced problem, Steihaug-Toint CG on
 * A p = -g in ONE engine call: the kept points are checked once, every reduction has a fixed order, every decision is made on the device.
 *   A = M (T' H(Z; sigma, mu~) T) M + shift M, with T, mu~ and the dependent set S as in "Reduced-space operators" above;
 *   M zeroes the entries of S and every entry i with free_mask[i] == 0.0 (free_mask [n_vars] doubles, NULL: all free; the mask of an S
 *   entry is not read, a NaN there reaches nothing);  g = M (dto_reduced_gradient at (Z, sigma, mu)).
 * The loop, from p = 0:
 *     r = g, d = -r, rr = r . r;  rr == 0: CONVERGED with 0 iterations
 *     iteration j = 1 .. max_iter:
 *       y = T'HT d                                   (dto_reduced_hessian_product's bits, same "reduced_input_store" setting)
 *       w = M (y + shift * d)
 *       kappa = d . w, dd = d . d, pd = p . d, pp = p . p
 *       kappa or rr not finite: NOT_FINITE, stop (p and r stay)
 *       kappa <= 0: NEG_CURVATURE;  s = tau with radius > 0, else s = 1 in iteration 1 and 0 later;  p = p + s * d, r = r + s * w, stop
 *       alpha = rr / kappa
 *       radius > 0 and (pp + (2 * alpha) * pd) + (alpha * alpha) * dd >= radius * radius: BOUNDARY;  s = tau;  p = p + s * d, r = r + s * w, stop
 *       s = alpha;  p = p + s * d, r = r + s * w, rr' = r . r
 *       sqrt(rr') <= max(atol, rtol * sqrt(rr0)): CONVERGED, stop              (rr0 = g . g)
 *       beta = rr' / rr, d = beta * d - r, rr = rr'
 *     after max_iter iterations: MAX_ITER
 *   tau = (-pd + sqrt(pd * pd + dd * (radius * radius - pp))) / dd, the step to the trust-region boundary.
 * Every product, sum, difference, quotient and square root above is rounded on its own, never contracted, in the operand order written
 * (csrc/dto_newton_plan.h holds the decision as one function, newton_decide, that the kernel calls).  A dot x . y over n_vars entries has
 * a fixed order: the entries are cut into chunks of 256; in chunk b lane l (0 .. 63) starts from a_l = 0 and adds x_i * y_i over
 * i = 256 b + l, + 64, .. ascending; the 64 lane sums are combined by the halving tree stated for the input-block product above
 * (a_l += a_{l+32}, .. , a_l += a_{l+1}), P_b = a_0; one wavefront then combines the P_b the same way, lane l adding P_b over b = l,
 * l + 64, .. ascending, then the halving tree.  No atomics; entries of S and masked entries hold exact zeros in r, d, w and p.  The step
 * therefore equals the same loop written in NumPy around dto_reduced_hessian_product, bit for bit, and repeated calls and both
 * entry-point families return the same bits.
 * Outputs.  p [n_vars]: the step, exactly 0 on S and on masked entries; it must not overlap Z or the mask.  info [8]:
 *   [0] the status (DTO_NEWTON_*)   [1] iterations run   [2] ||g|| = sqrt(rr0)   [3] the final ||r|| = sqrt(r . r)   [4] ||p|| = sqrt(p . p)
 *   [5] p . g   [6] the predicted decrease -0.5 * (p . g + p . r), which is -(g'p + p'Ap / 2) because r = g + A p holds on every exit
 *   [7] the last kappa / dd (0 without an iteration)
 * trace: NULL, or [max_iter][4] with kappa, dd, s, rr' (r . r behind the update) per iteration run; later rows are left untouched.
 * Points and costs.  The reduced point, the solves' point and the Hessian point are checked once per call, as by the block products; the
 * call leaves them as a single product at (Z, sigma, mu) would.  An iteration is the launches of one kept-point single product (on the
 * default route J v^ and J' w run once per iteration), three small launches and one 16-byte readback of (status, iterations); a call
 * adds two launches and one readback before the first iteration.
 * Workspaces, grow-only and allocated before anything is enqueued: 3 n_vars + 8 ceil(n_vars / 256) + 16 doubles, the block products'
 * for one column, and for the host-pointer form 2 n_vars + 8 + 4 max_iter doubles.
 * Refused with text, the handle stays usable and nothing is enqueued: what dto_reduced_hessian_product refuses; max_iter < 1; a negative
 * or non-finite radius, rtol or atol; a non-finite shift; Z, p or info = NULL.  The host-pointer form uploads, runs the device routine on
 * the handle's stream, downloads and blocks.  The _dev form takes device pointers (dmu, dfree_mask and dtrace may be NULL), works on
 * `stream`, waits on the readbacks named above and defers device-side errors like every _dev call. */
#define DTO_NEWTON_CONVERGED 0
#define DTO_NEWTON_BOUNDARY 1
#define DTO_NEWTON_NEG_CURVATURE 2
#define DTO_NEWTON_MAX_ITER 3
#define DTO_NEWTON_NOT_FINITE 4
int dto_projected_newton_step(dto_handle* h, const double* Z, double sigma, const double* mu, const double* free_mask, double radius,
                              double shift, double rtol, double atol, int32_t max_iter, double* p, double* info, double* trace);
int dto_projected_newton_step_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* dfree_mask, double radius,
                                  double shift, double rtol, double atol, int32_t max_iter, double* dp, double* dinfo, double* dtrace, void* stream);

/* ---- Bound-constrained truncated-Newton step: the step above with simple bounds lo <= Z + p <= hi on the independent entries (the
 * drives' derivatives, the timesteps, the states of knot 1, the drives where no DerivativeIntegrator eliminates them).  A step that would
 * leave the box stops at the face, the entries that reached it are fixed there, and the solve goes on along the face; a direction of
 * non-positive curvature is followed to the face.  One engine call; A, M, g, T, mu~ and S as above.
 *   lo, hi [n_vars] doubles, either may be NULL (all -inf / all +inf); the entries of S and the masked entries are not read.  lo_i > hi_i
 *   on a free entry is the caller's error and is not detected: the rules below still define the result.
 * Entry states, one code per entry (the optional output entry_state holds them as doubles, and can be passed back as the next call's
 * free_mask: every non-zero is free to be decided again):
 *   0 fixed (in S, or free_mask[i] == 0.0)   1 free   2 / 3 held at the lower / upper bound from the start
 *   4 / 5 hit the lower / upper bound during the call
 * F0 is the set of entries in state 1 behind the start (later in state 1, 4 or 5), F the set in state 1 now; F only shrinks.
 * The loop, from p = 0:
 *     an entry that is not fixed:  Z_i <= lo_i and g_i > 0: state 2 (tested first);  Z_i >= hi_i and g_i < 0: state 3;  otherwise state 1
 *     r = g on F0, 0 elsewhere;  d = -r;  rr0 = rr = r . r;  rr == 0: CONVERGED with 0 iterations
 *     iteration j = 1 .. max_iter:
 *       y = T'HT d                                   (dto_reduced_hessian_product's bits, same "reduced_input_store" setting)
 *       w = y + shift * d on F0, 0 elsewhere         (r is kept on all of F0: r = g + A0 p stays true there, A0 = A restricted to F0)
 *       kappa = d . w, dd = d . d, pd = p . d, pp = p . p
 *       t_i, for i in F with d_i != 0:  max(0, (hi_i - (Z_i + p_i)) / d_i) for d_i > 0,  max(0, (lo_i - (Z_i + p_i)) / d_i) for d_i < 0
 *       tau_box = the smallest t_i that is no NaN, +inf where there is none
 *       (status, s) = the decision of the step above from kappa, dd, pd, pp, rr, radius (NOT_FINITE, NEG_CURVATURE, BOUNDARY or "go on"
 *                     with s = alpha);  NOT_FINITE: stop (p and r stay)
 *       NEG_CURVATURE, radius == 0 and tau_box finite:  s = tau_box and the solve goes on
 *       otherwise s > tau_box:                           s = tau_box and the solve goes on         (BOUNDARY and NEG_CURVATURE included)
 *       p = p + s * d, r = r + s * w on every entry;  then for i in F, with t_i from the p before the update:
 *         d_i > 0 and (t_i <= s or Z_i + p_i >= hi_i):  p_i = hi_i - Z_i, state 5
 *         d_i < 0 and (t_i <= s or Z_i + p_i <= lo_i):  p_i = lo_i - Z_i, state 4           n_hit = the entries fixed so
 *       (r is not corrected for the rounding of a clamp)
 *       rr' = r . r over the new F;  p . g (g on F0), p . r, p . p over all entries
 *       BOUNDARY or NEG_CURVATURE: stop
 *       sqrt(rr') <= max(atol, rtol * sqrt(rr0)): CONVERGED, stop
 *       n_hit > 0: restart, d = -r on F and 0 elsewhere;  otherwise beta = rr' / rr, d = beta * d - r, and 0 on states 4 and 5;  rr = rr'
 *     after max_iter iterations: MAX_ITER
 * Each iteration is a CG step or takes at least one entry out of F, so the loop ends; a step of length 0 (tau_box = 0) is legal and
 * costs one product.  Every new product, sum, difference and quotient is rounded on its own in the operand order written; the dots have
 * the order stated above; a minimum and the integer counts are exact in any order (csrc/dto_newton_box_plan.h holds the rules as
 * functions the kernels call -- newton_box_classify, newton_box_breakpoint, newton_box_decide, newton_box_update -- and the loop as a
 * host program).  The step therefore equals the same loop written in NumPy around dto_reduced_hessian_product, bit for bit.  With
 * lo = -inf and hi = +inf everywhere (or both NULL), p, info [0 .. 7] and the first four columns of the trace are
 * dto_projected_newton_step's, bit for bit.
 * Outputs.  p [n_vars]: exactly 0 outside F0.  info [12]:
 *   [0 .. 7] as above, with [2] = sqrt(rr0) over F0, [3] the final sqrt(rr') over the final F, [6] = -0.5 * (p . g + p . r) with r on F0
 *   [8] the entries held at a bound from the start   [9] the entries hit   [10] the restarts   [11] |F| at exit
 * trace: NULL, or [max_iter][6] with kappa, dd, s, rr', tau_box, n_hit per iteration run; later rows are left untouched.
 * entry_state: NULL, or [n_vars] doubles holding the codes.  Zp: NULL, or [n_vars] with Z_i + p_i, except that the entries in state
 * 4 / 5 hold lo_i / hi_i EXACTLY: the point to hand to dto_feasible_merit next.  p, Zp and entry_state must not overlap Z, the mask or
 * the bounds.
 * Points and costs.  As above: the three kept points are checked once; an iteration is the launches of one kept-point single product,
 * three small launches (profile name "newton_box") and one 16-byte readback; a call adds two launches and one readback before the
 * first iteration.  The state codes live in one byte per entry on the device.
 * Workspaces, grow-only and allocated before anything is enqueued: 3 n_vars + 12 ceil(n_vars / 256) + 16 + ceil(n_vars / 8) doubles, the
 * block products' for one column, and for the host-pointer form 6 n_vars + 12 + 6 max_iter doubles.
 * Refused with text, the handle stays usable and nothing is enqueued: what dto_projected_newton_step refuses; p or info = NULL; p, Zp or
 * entry_state overlapping Z, free_mask, lo or hi.  The two forms behave as above (dlo, dhi, dentry_state and dZp may be NULL). */
#define DTO_BOX_FIXED 0
#define DTO_BOX_FREE 1
#define DTO_BOX_HELD_LOWER 2
#define DTO_BOX_HELD_UPPER 3
#define DTO_BOX_HIT_LOWER 4
#define DTO_BOX_HIT_UPPER 5
int dto_projected_newton_step_box(dto_handle* h, const double* Z, double sigma, const double* mu, const double* free_mask, const double* lo,
                                  const double* hi, double radius, double shift, double rtol, double atol, int32_t max_iter, double* p,
                                  double* info, double* trace, double* entry_state, double* Zp);
int dto_projected_newton_step_box_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* dfree_mask, const double* dlo,
                                      const double* dhi, double radius, double shift, double rtol, double atol, int32_t max_iter, double* dp,
                                      double* dinfo, double* dtrace, double* dentry_state, double* dZp, void* stream);

/* ---- Augmented-Lagrangian terms: the reduced-space calls above with a penalty on the non-dynamics rows (the knot constraints), so that
 * the trust-region loop of dto_projected_newton_step_box / dto_feasible_merit becomes the inner loop of an augmented-Lagrangian method.
 * A non-dynamics row r is an equality row (g_r = 0) or an inequality row (g_r <= 0) by its constraint's `equality` flag
 * (dto_constraint_bounds reports it); it has a multiplier mu_r and a penalty rho_r.  The row rules (Powell, Hestenes, Rockafellar;
 * csrc/dto_auglag_plan.h holds them as the function al_row the kernels call, every product, sum and quotient rounded on its own):
 *     rho_r == 0                       psi = mu g,  mult = mu,  weight = 0            (the row is not penalised, as in the calls above)
 *     s = mu + rho g
 *     equality row, or s > 0           psi = (mu + (0.5 rho) g) g,  mult = s,  weight = rho          (active)
 *     inequality row, s <= 0           psi = -(mu mu) / (2 rho),    mult = 0,  weight = 0            (inactive)
 *     viol = |g| (equality), max(0, g) (inequality);  a NaN in g, mu or rho, or rho < 0, gives NaN in psi, mult and weight
 * mult = psi'(g), weight = psi''(g).  P = sum_r psi_r is summed in dto_feasible_merit's order (lane l of 64 adds r = n_dyn + l, + 64, ..,
 * then the halving tree), so with every rho_r = 0 the merit below has dto_feasible_merit's bits.
 *   mu, rho [n_cons] doubles; the dynamics rows are not read.  mu may be NULL (zeros).  rho == NULL means no penalties: every call then
 *   makes the launches, and returns the bits, of the call it extends (named with each).
 *   info [8]: [0] P  [1] active rows  [2] max viol  [3] sum viol^2  [4] max |mult - mu|  [5] penalised rows (rho != 0)  [6], [7] 0;
 *   the maxima are exact and the counts integers held in doubles.
 * dto_auglag_rows: the row pass at Z.  mu_eff [n_cons]: mult in the non-dynamics rows (the first-order multiplier update), 0 in the
 *   dynamics rows; weight [n_cons] likewise; any of mu_eff, weight, info may be NULL.  The rows of g come from the constraints' value
 *   kernels alone: no sweep and no chain runs.
 * dto_auglag_merit: Phi = sigma f(Zf) + P(g(Zf)), Zf = the feasible trajectory of Z; dto_feasible_merit with the row pass in place of its
 *   sum (rho == NULL: dto_feasible_merit itself, info is then left untouched).  Zf, g, info optional.
 * dto_auglag_gradient: the reduced gradient of Phi: dto_reduced_gradient at mu_eff, bit for bit (rho == NULL: dto_reduced_gradient at mu;
 *   mu_eff is then mu with its dynamics rows zeroed).  lam, mu_eff optional.
 * dto_auglag_hessian_products: Y = T'(H(Z; sigma, mu~_eff) + J_c' W J_c) T V for n_cols vectors, J_c the non-dynamics rows of the Jacobian
 *   and W = diag(weight): dto_projected_hessian_products at mu_eff, with the Gauss-Newton term t_j = J_c' (W (J_c z^_j)) added to
 *   q_j = H z^_j by one rounded addition before q_S is gathered.  The bits of t_j are those of dto_eval_jacobian_product (non-dynamics
 *   rows), the scaling weight_r * c_r and dto_eval_jacobian_transpose_product of [0; c] on the same handle: a row's sum in the knot
 *   kernels' component order (pattern entries only), the constraints in list order, a constraint that repeats a knot walking its
 *   listings in order; on a handle whose products take the value-slab route, the slab products themselves.  Column c has the bits of
 *   the call with that column alone.  (rho == NULL: dto_projected_hessian_products.)
 * dto_auglag_newton_step: dto_projected_newton_step_box with that operator and that gradient; arguments, outputs, info [12] and trace as
 *   there, NULL bounds mean none.  (rho == NULL: dto_projected_newton_step_box.)
 * Points and costs.  A call runs the row pass once (one launch and the constraints' value kernels), then works at the three kept points
 *   of the call it extends with mu_eff as the multipliers: the points compare contents, so a second call at the same (Z, sigma, mu, rho)
 *   rebuilds nothing.  A chunk of w columns adds one launch per constraint ||v|| - c or ||v||^2 - c whose times and comps repeat nothing,
 *   whatever w is, and one addition launch; a quadratic-form constraint and a constraint that repeats a knot or a component go through
 *   the single-column product kernels, one column at a time.  Profile name "auglag".
 * Refused with text, the handle stays usable and nothing is enqueued: what the extended call refuses; a handle with a host-evaluated
 *   constraint (global constraints are among these); in the host-pointer forms a rho_r that is negative or a NaN, naming the row; outputs
 *   that overlap inputs.  The _dev forms take device pointers and work on `stream`, errors deferred as for every _dev call. */
int dto_auglag_rows(dto_handle* h, const double* Z, const double* mu, const double* rho, double* mu_eff, double* weight, double* info);
int dto_auglag_rows_dev(dto_handle* h, const double* dZ, const double* dmu, const double* drho, double* dmu_eff, double* dweight, double* dinfo,
                        void* stream);
int dto_auglag_merit(dto_handle* h, const double* Z, double sigma, const double* mu, const double* rho, double* phi, double* Zf, double* g,
                     double* info);
int dto_auglag_merit_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* drho, double* dphi, double* dZf, double* dg,
                         double* dinfo, void* stream);
int dto_auglag_gradient(dto_handle* h, const double* Z, double sigma, const double* mu, const double* rho, double* grad, double* lam, double* mu_eff);
int dto_auglag_gradient_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* drho, double* dgrad, double* dlam,
                            double* dmu_eff, void* stream);
int dto_auglag_hessian_products(dto_handle* h, const double* Z, double sigma, const double* mu, const double* rho, int32_t n_cols, const double* V,
                                double* Y);
int dto_auglag_hessian_products_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* drho, int32_t n_cols,
                                    const double* dV, double* dY, void* stream);
int dto_auglag_newton_step(dto_handle* h, const double* Z, double sigma, const double* mu, const double* rho, const double* free_mask,
                           const double* lo, const double* hi, double radius, double shift, double rtol, double atol, int32_t max_iter, double* p,
                           double* info, double* trace, double* entry_state, double* Zp);
int dto_auglag_newton_step_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* drho, const double* dfree_mask,
                               const double* dlo, const double* dhi, double radius, double shift, double rtol, double atol, int32_t max_iter,
                               double* dp, double* dinfo, double* dtrace, double* dentry_state, double* dZp, void* stream);

/* ---- Preconditioned truncated-Newton step: dto_auglag_newton_step (without rho: dto_projected_newton_step_box) with an L-BFGS
 * preconditioner built from pairs (s, y) -- automatic preconditioning after Morales and Nocedal: the pairs (d_j, A d_j) that CG forms
 * anyway define a limited-memory BFGS inverse, and the next solve is preconditioned with it.  The rules, once, in plain C++:
 * csrc/dto_precond_plan.h (the kernels of csrc/dto_precond.hip, the host routine and a g++-built test compile that text); every
 * operation is rounded on its own and every dot takes the truncated-Newton step's order, so a NumPy restatement has the same bits.
 * Pair store.  dto_set_option("newton_pairs", m), m = 0 .. 16, sets the capacity; 0, the default, means off; setting it clears the
 *   store.  Pairs are raw vectors in the Z layout, the newest last, in two banks of 2 m vectors each (2 * 2 m * n_vars doubles of
 *   device memory, allocated by the first push or harvest).  dto_newton_pairs_push appends one pair and drops the oldest at capacity;
 *   dto_newton_pairs_clear empties the store; dto_newton_pairs_info returns the count and the capacity (either may be NULL).
 * Preparation, once per call, with F0 the entries that are free behind the start: the Gram entries SY_ij = sum over F0 of s_i y_j and
 *   YY_ij (i <= j) and SS_ii; a pair is admitted, walking from the oldest, iff SY_ii, SS_ii, YY_ii are finite and
 *   SY_ii > 2^-26 sqrt(SS_ii YY_ii); gamma = SY_kk / YY_kk of the newest admitted pair k (none admitted: the identity).
 * Application z = P_F H P_F r, F the entries free now, the compact form of Byrd, Nocedal and Schnabel in one pass of independent dots:
 *   u = S~' r_F, v = Y~' r_F;  a = R^-1 u;  c1 = R^-T ((D + gamma YY) a - gamma v), c2 = -a;
 *   z_i = gamma r_i + sum_k c1_k s_k,i + gamma sum_k c2_k y_k,i on F and 0 elsewhere, R the upper triangle and D the diagonal of SY over the
 *   admitted pairs.  A principal submatrix of a positive definite matrix: no Gram matrix is rebuilt when an entry hits a bound.
 * dto_newton_precondition: z_c = P H P r_c for n_cols vectors [n_cols][n_vars] at the store as it stands, F0 = F = the independent
 *   entries that free_mask (NULL: all) leaves.  Column c has the bits of the call with that column alone.
 * dto_preconditioned_newton_step: the arguments of dto_auglag_newton_step, then `harvest` in front of the outputs.  rho == NULL: the
 *   operator of dto_projected_newton_step_box; lo == hi == NULL: no bounds.  The loop is the box step's with these changes and no
 *   others: z is formed from r behind the start and behind every update; rz = r . z over F takes rr's place in alpha = rz / kappa and
 *   beta = rz' / rz; d = beta d - z, the start is d = -z and a restart d = -z on F.  The convergence test, the reach, tau, tau_box, the
 *   clamps, the predicted decrease and info[0 .. 11] keep their Euclidean definitions, and the trust region stays the Euclidean ball:
 *   ||p|| is no longer monotone under preconditioning, but a boundary step still decreases the model, since q is convex and decreasing
 *   on [0, alpha] along d.  Fallback: where the loop goes on with rz' not finite or <= 0, the preconditioner is switched off for the
 *   rest of the call, rz' = rr', d = -r on F, and one fallback is counted.
 *   info [16]: the box step's 12, then the pairs admitted, the pairs taken by the harvest, the fallbacks, sqrt(rz0).
 *   trace [max_iter][8]: the box step's six columns, rz' as formed, and 1 / 0: the preconditioner is on / off behind the iteration.
 *   harvest != 0: iteration j offers (d, w) as the loop holds them, w = y + shift d on F0; the pair is taken iff kappa is finite
 *   and > 0.  The other bank keeps the last min(m, taken) pairs, and when the call ends, whatever its exit, the banks swap if a pair was
 *   taken.  The call never reads a pair it wrote.
 *   Identity: with an empty store, or with no pair admitted, z = r and rz = rr bit for bit, and p, info[0 .. 11], the trace's six
 *   columns, entry_state and Zp are dto_projected_newton_step_box's (with rho: dto_auglag_newton_step's) bit for bit.
 * Costs.  Per call the box start, one Gram launch, one one-workgroup launch (stage 2, admission, R, M), and the first application (multi-dot
 *   launch, combination launch).  Per iteration the product and four launches: the box step's curvature pass; the step, which also
 *   copies a harvested pair and runs the multi-dot pass on the r it has just updated; the combination (every workgroup finishes the 2 m
 *   dots and runs the two triangular solves itself, then writes z); the direction.  An application reads each stored vector twice.
 *   Profile name "precond" (every launch of these calls that is no product).
 * Refused with text, the handle stays usable and nothing is written: what dto_auglag_newton_step refuses (the penalty rules with rho
 *   only); a push, or harvest != 0, while the capacity is 0; newton_pairs outside 0 .. 16; in dto_newton_pairs_push a non-finite
 *   entry, naming it; n_cols < 1; outputs that overlap inputs.  The _dev forms take device pointers and work on `stream`, errors
 *   deferred as for every _dev call; the store is read and written in stream order, so pushes and steps belong on one stream. */
int dto_newton_pairs_push(dto_handle* h, const double* s, const double* y);
int dto_newton_pairs_push_dev(dto_handle* h, const double* ds, const double* dy, void* stream);
int dto_newton_pairs_clear(dto_handle* h);
int dto_newton_pairs_info(dto_handle* h, int32_t* count, int32_t* capacity);
int dto_newton_precondition(dto_handle* h, const double* free_mask, int32_t n_cols, const double* r, double* z);
int dto_newton_precondition_dev(dto_handle* h, const double* dfree_mask, int32_t n_cols, const double* dr, double* dz, void* stream);
int dto_preconditioned_newton_step(dto_handle* h, const double* Z, double sigma, const double* mu, const double* rho, const double* free_mask,
                                   const double* lo, const double* hi, double radius, double shift, double rtol, double atol, int32_t max_iter,
                                   int32_t harvest, double* p, double* info, double* trace, double* entry_state, double* Zp);
int dto_preconditioned_newton_step_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* drho, const double* dfree_mask,
                                       const double* dlo, const double* dhi, double radius, double shift, double rtol, double atol,
                                       int32_t max_iter, int32_t harvest, double* dp, double* dinfo, double* dtrace, double* dentry_state,
                                       double* dZp, void* stream);

/* ---- Reduced-space minimize: the trust-region loop around the step and the merit above, and with penalties the outer multiplier /
 * penalty loop around that, as ONE call that stays on the device.  The rules, once, in plain C++: csrc/dto_minimize_plan.h (the kernels
 * of csrc/dto_minimize.hip, the host routine and a g++-built test compile that text); every operation is rounded on its own, so a NumPy
 * restatement around the public step, merit and row pass has the same bits.  The call composes the existing routines unchanged:
 *   step    dto_preconditioned_newton_step where the capacity "newton_pairs" is above 0, else dto_auglag_newton_step (rho == NULL:
 *           dto_projected_newton_step_box), with radius = delta and the options' shift, rtol, atol, max_iter;
 *   merit   dto_auglag_merit (rho == NULL: dto_feasible_merit);      rows    dto_auglag_rows.
 * A trial:  (info, Zp) = step(Z, delta).  info[2] = ||g|| <= gtol ends the inner loop with GRADIENT before any merit is evaluated; the
 *   step is discarded and the trial logged as rejected.  Otherwise (phi_t, Zt) = merit(Zp) and, minimize_trial_decide,
 *     ratio = (phi - phi_t) / predicted;   accepted = ratio > eta_accept: Z = Zt, phi = phi_t;
 *     ratio < eta_shrink: delta / shrink_div;  else ratio > eta_grow and the step's status != DTO_NEWTON_CONVERGED:
 *     min(delta * grow_mul, radius_max);  else delta.
 *   The step's status DTO_NEWTON_NOT_FINITE, or a ratio that is not finite (predicted == 0 among these), ends the call with NOT_FINITE:
 *   the trial is rejected and delta stays.  A new delta below radius_min ends the inner loop with RADIUS, the last trial with MAX_TRIALS.
 * An outer iteration (rho != NULL; without rho there is exactly one, with no row pass and no outer decision):  phi, Z <- merit(Z), so Z
 *   becomes its feasible trajectory; delta = radius0; up to `trials` trials; then, unless the call ended NOT_FINITE, the row pass at Z
 *   gives mu_eff and max viol, mu <- mu_eff on the non-dynamics rows, and minimize_outer_decide:
 *     grew = !(new_viol <= viol / viol_div)  (a NaN grows the penalty): rho_r <- rho_r * rho_mul on the rows with rho_r != 0;
 *   viol = new_viol.  The first viol is the row pass's at the caller's Z.  Dynamics rows of mu and rho are never written.
 * Exit status, info[0]:  DTO_MINIMIZE_CONVERGED  the inner loop ended with GRADIENT and, with rho, max viol <= ctol;
 *   DTO_MINIMIZE_MAX_OUTER  `outer` ran out;  DTO_MINIMIZE_NOT_FINITE;  and without rho only DTO_MINIMIZE_MAX_TRIALS, DTO_MINIMIZE_RADIUS.
 *   With gtol = ctol = radius_min = 0, the defaults, the loop runs outer x trials trials (unless a gradient norm is exactly 0).
 * options [16] (NULL: the defaults), indices DTO_MIN_OPT_*:  radius0 (1), eta_accept (0.1), eta_shrink (0.25), eta_grow (0.75),
 *   shrink_div (4), grow_mul (2), radius_max (+inf), radius_min (0), gtol (0), ctol (0), viol_div (4), rho_mul (10), and the step's
 *   shift (0), rtol (1e-6), atol (0), max_iter (50).  The defaults make the loops of the README, bit for bit.
 * info [16]:  status, outer iterations, trials, accepted trials, phi first, phi last, the last delta, the last step's ||g||, max viol
 *   first, max viol last, penalty increases, the sum of the steps' CG iterations, pairs harvested, fallbacks, 0, 0.
 * history [outer * trials][8] (or NULL), one row per trial run, consecutive:  ratio, accepted, the delta used, phi_t, predicted, the
 *   step's status, iterations and ||g||  (a GRADIENT trial: ratio 0, phi_t = phi).  outer_history [outer][4] (or NULL):  max viol, grew,
 *   active rows, P.  Rows the loop does not reach keep the caller's values.  entry_state [n_vars] (or NULL): the last step's.
 * Z, mu and rho are in / out (mu may be NULL only where rho is; without rho mu is an input).  harvest as in the preconditioned step.
 * Costs.  Two kernels of dto_minimize.hip, profile name "minimize": one launch behind every trial (every workgroup takes the decision
 *   itself and copies its slice of Zt into Z where the trial is accepted; workgroup 0 writes the scalars, the history row and a
 *   32-byte mailbox), one behind every outer iteration (mu, rho, the scalars).  The scalars live in two banks, so no launch reads a
 *   scalar it writes.  The host reads the mailbox (accepted, delta, stop, phi) once per trial -- it needs delta as the next step's radius
 *   -- and the step's 24 bytes (status, iterations, ||g||) in front of the merit for the gradient test; no vector crosses the bus
 *   between the upload and the download of the host-pointer form.  A rejected trial leaves Z's contents alone, so the next step finds
 *   its kept points and rebuilds nothing.
 * Refused with text, with nothing enqueued: what the composed calls refuse (sharded handles among these); outer < 1 or trials < 1;
 *   rho == NULL with outer != 1; rho != NULL with mu == NULL; radius0 <= 0 or not finite; a negative or NaN option; not
 *   0 <= eta_accept <= eta_shrink < eta_grow; shrink_div <= 1 or grow_mul < 1; a max_iter that is no whole number; harvest with
 *   capacity 0; outputs that overlap inputs or each other.  The _dev form takes device pointers, updates dZ, dmu and drho in place on
 *   `stream` and waits for its mailbox on it; `options` is a host pointer in both forms; errors are deferred as for every _dev call. */
#define DTO_MINIMIZE_CONVERGED 0
#define DTO_MINIMIZE_MAX_OUTER 1
#define DTO_MINIMIZE_MAX_TRIALS 2
#define DTO_MINIMIZE_RADIUS 3
#define DTO_MINIMIZE_NOT_FINITE 4
#define DTO_MIN_OPT_RADIUS0 0
#define DTO_MIN_OPT_ETA_ACCEPT 1
#define DTO_MIN_OPT_ETA_SHRINK 2
#define DTO_MIN_OPT_ETA_GROW 3
#define DTO_MIN_OPT_SHRINK_DIV 4
#define DTO_MIN_OPT_GROW_MUL 5
#define DTO_MIN_OPT_RADIUS_MAX 6
#define DTO_MIN_OPT_RADIUS_MIN 7
#define DTO_MIN_OPT_GTOL 8
#define DTO_MIN_OPT_CTOL 9
#define DTO_MIN_OPT_VIOL_DIV 10
#define DTO_MIN_OPT_RHO_MUL 11
#define DTO_MIN_OPT_SHIFT 12
#define DTO_MIN_OPT_RTOL 13
#define DTO_MIN_OPT_ATOL 14
#define DTO_MIN_OPT_MAX_ITER 15
#define DTO_MIN_OPTIONS 16
int dto_projected_minimize(dto_handle* h, double* Z, double sigma, double* mu, double* rho, const double* free_mask, const double* lo,
                         const double* hi, const double* options, int32_t outer, int32_t trials, int32_t harvest, double* info, double* history,
                         double* outer_history, double* entry_state);
int dto_projected_minimize_dev(dto_handle* h, double* dZ, double sigma, double* dmu, double* drho, const double* dfree_mask, const double* dlo,
                             const double* dhi, const double* options, int32_t outer, int32_t trials, int32_t harvest, double* dinfo,
                             double* dhistory, double* douter_history, double* dentry_state, void* stream);

/* ---- Multi-GPU: knot ranges sharded over the GPUs of one node, one process (or thread with its own device) per GPU
 * (BASELINE configs[3] "knot range sharded across 8 x MI355X (RCCL allgather)").  The engine owns the RCCL
 * communicator (SURVEY.md §8b "Ownership").  No callback needs a collective: every rank's Jacobian / Hessian / gradient
 * output is one contiguous slab of the global value vector.  The entry points below serve a consumer that wants the WHOLE
 * vector on every GPU (MadNLP's KKT assembly in GPU mode, ext/MadNLPSolverExt/solver.jl:81,
 * src/solvers/madnlp_solver/options.jl:12-16) and the objective's sum over the ranks.
 *
 *   1. one rank:   dto_comm_unique_id(id)                  -- hand the 128 bytes to the others (MPI, a file, a socket)
 *   2. every rank: dto_comm_create(h, id, rank, world)     -- collective; exchanges the ranks' knot ranges
 *   3. every rank: dto_get_gather_layout(h, DTO_VECTOR_JACOBIAN, &L); allocate L.padded_len doubles of device memory `buf`;
 *                  the global value vector is buf + L.front_pad, this rank's slab starts at buf + L.front_pad + L.own_lo
 *   4. per call:   dto_eval_jacobian_dev(h, dZ, buf + L.front_pad + L.own_lo, stream);
 *                  dto_gather_jacobian_dev(h, buf, stream);   -- all ranks, same order; enqueued on `stream`
 *
 * With contiguous knot ranges in rank order the gather is ONE in-place ncclAllGather on `buf` (L.in_place_all_gather = 1:
 * the first and the last rank's slabs are a boundary half-block shorter than the others, which is what front_pad and the
 * padding behind the vector absorb -- a few hundred KB on 17.6 GB); any other assignment of knots to handles (a rank's knots
 * over two handles to overlap the gather of one with the compute of the other) is served by one in-place ncclBroadcast per
 * rank inside a group call, and padded_len = total.  Padding is never read as data.
 * dto_comm_set_ranges is the same bookkeeping WITHOUT a communicator (also on structure-only handles): for callers that move
 * the slabs with a transport of their own and only want the layout. */
#define DTO_COMM_ID_BYTES 128
#define DTO_VECTOR_JACOBIAN 1
#define DTO_VECTOR_HESSIAN 2
#define DTO_VECTOR_GRADIENT 3
#define DTO_VECTOR_CONSTRAINT 4 /* g: a rank's rows are several segments of the global vector (dto_shard_rows), moved by
                                   one broadcast per segment; layout: total = n_cons, no padding, own_lo / own_len unused */
typedef struct dto_gather_layout {
    int64_t total;       /* length of the global vector */
    int64_t padded_len;  /* doubles to allocate */
    int64_t front_pad;   /* the global vector starts here inside the allocation */
    int64_t own_lo;      /* this rank's slab inside the global vector (= dto_shard_info.*_lo) */
    int64_t own_len;
    int32_t in_place_all_gather; /* 1: one ncclAllGather moves every slab; 0: one broadcast per rank */
    int32_t world;
} dto_gather_layout;
int dto_comm_unique_id(void* id128);
int dto_comm_create(dto_handle* h, const void* id128, int32_t rank, int32_t world);
int dto_comm_set_ranges(dto_handle* h, int32_t rank, int32_t world, const int64_t* k_lo, const int64_t* k_hi);
int dto_comm_destroy(dto_handle* h);
int dto_get_gather_layout(const dto_handle* h, int32_t vector, dto_gather_layout* out);
/* every rank's (lo, len) of one value vector, [world] each (VECTOR_JACOBIAN / HESSIAN / GRADIENT) */
int dto_gather_slabs(const dto_handle* h, int32_t vector, int64_t* lo, int64_t* len);
int dto_gather_jacobian_dev(dto_handle* h, double* dbuf, void* stream);
int dto_gather_hessian_dev(dto_handle* h, double* dbuf, void* stream);
int dto_gather_gradient_dev(dto_handle* h, double* dbuf, void* stream);
/* dg_full [n_cons]: the rank's local rows (dg_local, as dto_eval_constraint_dev wrote them) are copied to their global
 * positions, the other ranks' segments arrive by broadcast */
int dto_gather_constraint_dev(dto_handle* h, const double* dg_local, double* dg_full, void* stream);
/* *df := sum over the ranks of *df (the objective's per-shard partial sums, evaluator.jl:304); ncclAllReduce on `stream` */
int dto_allreduce_objective_dev(dto_handle* h, double* df, void* stream);

/* Bound outputs (device-pointer callbacks).  A solver in GPU mode hands the SAME device vector to eval_constraint_jacobian /
 * eval_hessian_lagrangian every iteration (MadNLP's callback buffers; ext/MadNLPSolverExt/solver.jl:81).  Half of a Jacobian slab
 * and ~99 % of a Hessian slab never change -- structural zeros the reference's `fill!(..., 0)` rewrites every call
 * (evaluator.jl:497, :571), the identity blocks of the z_{k+1} halves.  dto_bind_output_dev(h, DTO_VECTOR_JACOBIAN | _HESSIAN, ptr)
 * declares such a vector: the first dto_eval_*_dev call into `ptr` writes it in full, later calls into the same pointer write
 * only what can change (and clear only the runs that kernels accumulate into), PROVIDED the caller has not written the other
 * entries in between (it may read everything and overwrite the variable entries).  Calls with any other pointer, and all
 * host-pointer calls, keep the full-write semantics; ptr = NULL unbinds; a failed call re-arms the full write.
 * (-0.3 ms per Jacobian, -0.25 ms per Hessian at 256 states x 2000 knots: 1.1 GB / 1.7 GB of zero-fill less.) */
int dto_bind_output_dev(dto_handle* h, int32_t vector, double* dptr);

/* Options (name, value); unknown names are an error.
 *   "reuse_forward_sweep" (default 0): interior-point solvers evaluate g, J and H at the same point one after the
 *   other.  With this on, the engine remembers the forward generator sweep of the last callback and re-uses it when
 *   the next callback's Z is bit-identical (compared on the device, one 4-byte readback): eval_constraint after
 *   eval_jacobian then costs a copy, eval_jacobian after eval_constraint sweeps its tangent columns only, eval_hessian
 *   skips its forward sweep and -- after an eval_jacobian at that point -- takes the step budget that call's propagator chain
 *   planned from its exact norms instead of buying them again (a sixth of a Hessian at 1024 states).  Results agree to rounding
 *   either way (the constraint-only
 *   sweep sums its generator products in a different order than the Jacobian's); the benchmark never turns it on (each
 *   callback is timed cold). */
/*   "expm_form" (default 0): evaluation form of the matrix-exponential polynomial in eval_constraint_jacobian.  0 picks per
 *   call by cost: two products for the degree-16 Taylor polynomial (backward-error radius 0.78) or three products for an
 *   order-26 approximant (radius 2.82, i.e. up to two squarings fewer); 2 / 3 force one form (tests, measurements). */
/*   "host_xfer" (default 1): the host-pointer dto_eval_jacobian / dto_eval_hessian copy only the entries that can change
 *   from call to call (about half of a Jacobian slab, ~1 % of a Hessian slab) through a pinned ring and fill the constant
 *   entries (identity / zero runs) with host threads while the GPU computes; 0 copies the whole slab in one piece.  To be set
 *   before the first such call.
 *   "overlap_sweep" (default 1): eval_constraint_jacobian runs its generator sweep on a second stream next to the polynomial
 *   products and squarings of the propagator chain (5-6 % faster at 256 states x 2000 knots); 0 runs one kernel at a time,
 *   which is what per-kernel measurements (dto_profile_get, rocprofv3) need.  Results agree to rounding: bit-identical, except
 *   that next to the chain a 256-state sweep over 1536 intervals or more groups its intervals by twelve instead of nine (a
 *   different, equally fixed summation order of the generator products).
 *   "sweep_form" (default 0): 0 runs the generator sweep as one persistent launch where that form applies, 1 always one
 *   launch per Taylor step.
 *   "chain_form" (default 0): 0 runs the propagator chain of a 33..64-state integrator as ONE launch (a workgroup per interval, the
 *   evaluation form chosen per interval on the device), 1 always as batched-GEMM launches over all intervals (the form of larger
 *   integrators).  Same approximants and radii either way; results agree to rounding.
 *   "chain_chunk" (default 0 = the engine's workspace budget): at most this many intervals per chunk of the propagator
 *   chain (what a 16000-knot trajectory does by itself; tests use it to exercise the chunk loop on small problems).
 *   "host_xfer_check" (default 0): every host-pointer dto_eval_jacobian / dto_eval_hessian also copies the whole device slab and
 *   compares it bit for bit with the vector it assembled from the variable runs and the constants; a difference (a kernel that
 *   wrote an entry the hand-off plan does not list) fails the call.  The repository's GPU tests run with it on.
 *   "tdb_share_members" (default: the largest count the handle was created for): members per launch of an active group of
 *   time-dependent integrators (DTO_FLAG_SHARED_GENERATORS), 1 .. that count; 1 is one launch per member through the lone kernel,
 *   the A/B switch.  Values outside the range are refused.  The results do not depend on it, bit for bit.
 *   "tdb_resident" (default 0 = every integrator's own grid): upper bound on the workgroups of the persistent-grid launches of
 *   time-dependent integrators -- k_tdb_mfma, its group form and its matrix-free products, k_tdb_kron and its matrix-free products
 *   (k_tdb_kron_product) -- which by default start
 *   min(owned knots + 1, two per compute unit) workgroups that walk the intervals, one scratch slot each.  1 .. the largest such grid
 *   among the handle's integrators on these kernels caps the grid (a launch takes the smaller of the value and its own grid, and the
 *   first slots of the scratch it already has); values outside the range are refused, and a handle without such an integrator takes
 *   0 only.  For tests and measurements: a small problem then makes a workgroup walk several intervals.  The results do not depend
 *   on it, bit for bit.
 *   "tdb_matrix_free_products" (default 0): 1 makes dto_eval_jacobian_product / _transpose_product (and their _dev forms) of a handle
 *   with device TimeDependentBilinearIntegrators matrix-free, on every device path of theirs: the dense ones (1..256 states) and the
 *   structured one (DTO_FLAG_BLOCK_GENERATORS structure found and used: replicated-block generators, 33..512 states).  J w is the
 *   discrete scheme applied to two vectors, J' w to 1 + p forward vectors and one adjoint vector -- on the structured path to as
 *   many column groups of the b x b map -- with no propagator block, no staged Jacobian block, no value slab; a product then costs
 *   about a constraint call, not a Jacobian call.  Such a handle may mix structured and dense time-dependent integrators and also
 *   hold bilinear and derivative integrators and built-in knot constraints: it goes matrix-free as a whole.  External integrators
 *   and constraints keep the slab route whatever the option says.  0 leaves every call as it was; values other than 0 and 1 are refused.  Results of the two routes agree to rounding (another summation order).
 *   "reduced_input_store" (default 0): 1 makes dto_reduced_gradient / dto_reduced_hessian_product (and their _dev forms) take their
 *   J v^ and J' w from input blocks kept with dto_dynamics_solve_all's point ("Reduced-space operators" above states the store, the
 *   summation orders and the costs).  0 leaves every call as it was; values other than 0 and 1 are refused.
 *   "reduced_block_width" (default 0 = the engine's choice, 64): 1 .. 64 caps the columns per chunk of dto_eval_hessian_products /
 *   dto_projected_hessian_products and their _dev forms ("Block products" above); other values are refused.  For tests, which then
 *   exercise the chunk loop on small blocks, and for measurements.  The results do not depend on it, bit for bit.
 *   "newton_pairs" (default 0 = no preconditioner): 0 .. 16, the capacity of the pair store of dto_preconditioned_newton_step
 *   ("Preconditioned truncated-Newton step" above); other values are refused.  Setting it clears the store.
 *   "debug_bad_launch": TUNING builds only (libdto_engine_t.so) -- 1 gives the next callbacks' kernels an invalid launch
 *   configuration, which must come back as a non-zero return code with text (test of the error convention); the product
 *   library refuses the name. */
/*   "deterministic" (default 0).  Run to run the engine is bit-reproducible without any option: every reduction has a fixed
 *   order (column sums of the generator-subspace GEMMs per 64-row chunk, objective partial sums, listings of a term that
 *   repeats a knot layer by layer, contributions to global-variable entries in listing order; the sweeps' K order is a function
 *   of the block index).  What still depends on HOW a result is asked for is switched off by 1: the Jacobian's sweep keeps the
 *   interval grouping it has alone on the chip (else `overlap_sweep` changes the summation order at 256 states), the Hessian's
 *   forward p-column sweep runs after its adjoint sweep instead of beside it (else `overlap_sweep` switches that column between
 *   step launches and the generator-stationary form at 128 / 256 states, and regroups its intervals at 33..64), and the
 *   host-pointer dto_eval_jacobian runs the propagator chain in the same chunks as dto_eval_jacobian_dev (else the early
 *   hand-over of -E_k caps the chunk, and the evaluation form is decided per chunk).  Cost at 256 x 2000: +0.1..0.4 ms per
 *   device-resident Jacobian, and the host-pointer Jacobian loses the overlap of its PCIe copy with the chain (23 -> 34 ms).
 *   dto_eval_jacobian_product / _transpose_product are covered since round 4: every entry of y has one writer per launch with a
 *   fixed internal order (J w gathers row by row; J' w writes per knot, listings that repeat a knot in listing order). */
int dto_set_option(dto_handle* h, const char* name, int64_t value);

/* measurement hooks: HIP-event timing of the engine's kernels on the stream they are launched on */
int dto_profile_enable(dto_handle* h, int32_t on);
int dto_profile_reset(dto_handle* h);
/* name: "bgemm" (batched f64 MFMA GEMM of the propagator chain: every template instance), its parts
 * "bgemm_horner" (the products with a fused polynomial epilogue) / "bgemm_square" / "bgemm_plain" / "chain64" (the one-launch
 * chain of a 33..64-state integrator, priced at six products per interval), "basis"
 * (generator-subspace GEMM), "expmv" (forward generator sweeps and the pairing products), "expmv_adjoint" (the Hessian's adjoint
 * sweep: its dominant kernel), "all"; "basis_multi" / "basis_k" (the two generator-subspace launches apart: A^2..A^4, and the
 * factor K), and the bandwidth-bound assembly kernels "zero_fill" (the Jacobian's / Hessian's fill!(., 0)), "build_A" (A_k from the
 * generators), "assembly" (the writers of the bilinear Jacobian's tangent columns), "hess_product" (the Hessian-vector products'
 * gather into their compact copy and the product launches; the Hessian they assemble counts under its own names), "share" (the
 * copies of the leader's -E_k blocks to the followers of a DTO_FLAG_SHARED_GENERATORS group; its bytes are the bytes WRITTEN, one
 * block per follower and interval -- each launch reads a further block per interval -- and stay out of the third output of "all"),
 * "tdb_product" (the matrix-free J w / J' w of time-dependent integrators, option "tdb_matrix_free_products": one record per
 * integrator and product, dense or structured, flops as executed with padding; these launches do not count under "tdb_mfma" or
 * "tdb_kron"),
 * "rollout" (dto_rollout / dto_rollout_dev: the gather of the -E_k blocks, the tree's batched products and the descent, flops as
 * executed with padding; its parts "rollout_gather" / "rollout_tree" / "rollout_descent", the last with the start and the copy into
 * the caller's layout; the tree's products do not count under "bgemm" / "bgemm_plain", and these names feed no other, "all" included;
 * the Jacobian evaluation inside a rollout counts under its own names),
 * "dynsolve" (dto_dynamics_solve / dto_dynamics_solve_dev; its parts "dynsolve_tree", the gather and the tree's products of a rebuild
 * -- no launches at a cached point -- and "dynsolve_scan", the loader, the offsets' up-sweep, the descent and the copy into the
 * caller's layout; flops as executed with padding; like the rollout's these names feed no other, "all" included, and the Jacobian
 * evaluation inside a rebuild counts under its own names),
 * "dynsolve_couple" and "dynsolve_deriv" (dto_dynamics_solve_all / dto_dynamics_solve_all_dev: the gather of the coupling blocks with
 * the contractions against them, and the DerivativeIntegrators' block solves -- third output: BYTES as executed; the call's other
 * block solves count under "dynsolve_tree" and "dynsolve_scan"; neither name feeds another, "dynsolve" and "all" included),
 * "reduced_pack" (the packer launches of dto_reduced_gradient / dto_reduced_hessian_product and their _dev forms -- third output:
 * BYTES as executed; it feeds no other name, "all" included, and the routines the operators are made of count under their own names),
 * "reduced_input" (option "reduced_input_store": the gather of the input blocks at a rebuilt point, one launch per integrator with free
 * inputs, and the two products with them, one launch each -- third output: BYTES as executed; it feeds no other name, "all" included).
 * "feasible" (dto_feasible_trajectory / dto_feasible_merit and their _dev forms: the DerivativeIntegrators' recurrences, the scatters of
 * the rolled-out states into Zf and the merit sum, one launch each -- third output: BYTES as executed; it feeds no other name, "all"
 * included; the Jacobian evaluation inside counts under its own names, the trees and descents under "rollout_gather" / "rollout_tree" /
 * "rollout_descent").
 * "newton" (dto_projected_newton_step and its _dev form: the four kernels of the step -- start, curvature pass, step, direction update --
 * two launches per call and three per iteration; third output: BYTES as executed; it feeds no other name, "all" included; the products
 * of the iterations count as the block products do).
 * "newton_box" (dto_projected_newton_step_box and its _dev form: its four kernels, counted in the same way; no launch of it counts
 * under "newton").
 * "auglag" (the dto_auglag_* calls: the row pass, the Gauss-Newton term's launches, the scaling and the addition; third output: BYTES as
 * executed; it feeds no other name, "all" included; with rho == NULL no launch counts here).
 * "precond" (dto_preconditioned_newton_step, dto_newton_precondition, dto_newton_pairs_push_dev: every launch of theirs that is no
 * product -- the Gram pass, the preparation, the multi-dot and combination passes, the step and the direction, and the box step's start
 * and curvature pass where they run inside; third output: BYTES as executed; it feeds no other name, "all" included).
 * "minimize" (dto_projected_minimize and its _dev form: the two kernels of dto_minimize.hip, one launch per trial and one per outer
 * iteration; third output: BYTES, a trial's as if it is accepted; it feeds no other name, "all" included; the step, the merit and the
 * row pass inside count under their own names).
 * The block products count under "hess_product", "reduced_pack" and "reduced_input" too, one launch per chunk where a single product
 * has one, with bytes as executed: matrix bytes once per tile or chunk, vector bytes per column.
 * Returns accumulated device milliseconds, launches and algorithmic FLOPs of those launches -- for the four assembly names and "share" the
 * third output is the launches' algorithmic BYTES (what they must read and write), not FLOPs.
 * "hess_product_setup" returns the host milliseconds of the products' index build (once per handle), 0 launches, and the device
 * bytes of their private slab and index.
 * "sweep_gs" / "sweep_fused" / "sweep_s64" / "sweep_cluster" / "sweep_step": generator sweeps by the form they ran in
 * (generator-stationary, fused, the 64-state fused form, row-split cluster, one launch per Taylor step), one count per sweep
 * while profiling is on -- 0 ms, the count, 0 flops; they feed no other name ("all", "expmv", ...). */
int dto_profile_get(dto_handle* h, const char* name, double* ms, int64_t* launches, double* flops);
/* diagnostics of the last Jacobian call: max squarings used, Taylor terms used by the tangent sweep */
int dto_last_stats(const dto_handle* h, int32_t* max_squarings, int32_t* expmv_terms);

#ifdef __cplusplus
}
#endif
#endif /* DTO_ENGINE_H */
