// dto_handle.h -- what the engine's translation units share: the handle behind the C ABI (dto_engine.h), the host-side records it
// is made of, and the few helpers both creation (dto_create.cpp) and evaluation (dto_engine.cpp) call.  Private: not installed,
// not included from include/dto_engine.h.
#pragma once

#include "../../include/dto_engine.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "dto_comm.h"
#include "dto_elim_plan.h"
#include "dto_feasible_plan.h"
#include "dto_hostxfer.h"
#include "dto_input_plan.h"
#include "dto_kept_point.h"
#include "dto_kernels.h"
#include "dto_sweep_cache.h"

namespace dto {

extern thread_local std::string g_create_error;  // dto_last_error(nullptr): why the last dto_create of this thread failed

struct HipError {
    std::string msg;
};

#define HIP_CHECK(expr)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            char buf_[512];                                                                      \
            snprintf(buf_, sizeof(buf_), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                     __FILE__, __LINE__);                                                        \
            throw HipError{buf_};                                                                \
        }                                                                                        \
    } while (0)

template <class T>
T* dalloc(size_t n) {
    void* p = nullptr;
    if (n == 0) n = 1;
    HIP_CHECK(hipMalloc(&p, n * sizeof(T)));
    return static_cast<T*>(p);
}
template <class T>
T* dupload(const std::vector<T>& v) {
    T* p = dalloc<T>(v.size());
    if (!v.empty()) HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return p;
}

// Grow-only device workspace of a sweep form whose workgroups hand data to each other (ensure_sweep_work replaces both parts)
struct SweepWork {
    double* slab = nullptr;
    unsigned* arrive = nullptr;
    size_t cap = 0;     // doubles in slab
    int counters = 0;   // interval groups (generator-stationary) or clusters (row-split) the counters serve
};

struct BilHost {
    KBil k;
    SweepBuf fw{}, ad{};
    int T_alloc = 0;
    std::vector<double> g1;   // ||G_j||_1
    std::vector<double> n2;   // ||G_i G_j||_1, (m+1)^2
    double* d_g1 = nullptr;
    double* d_n2 = nullptr;
    ChainWork chain{};
    int chain_cap = 0;
    unsigned long long* d_hump = nullptr;  // [8] k_hump output: log hump(q), last term index, q = 1..4 (max over intervals)
    double hump_logH[4] = {0, 0, 0, 0};
    int hump_kend[4] = {0, 0, 0, 0};
    bool hump_valid = false;
    // option reuse_forward_sweep: what b.fw still holds for the cached Z, and the step budget the Jacobian's chain planned there
    // (dto_sweep_cache.h: written by one recorder per producer, read through cache.at(same) only)
    SweepCache cache;
    // row-split cluster sweeps (dto_sweep_fused.hip): exchange slabs and arrival counters, one set per sweep buffer ([0] fw,
    // [1] ad: the Hessian's forward and adjoint sweeps may run side by side)
    SweepWork cluster_work[2];
    // generator-stationary sweeps (dto_sweep_gs.hip): partial-norm slabs and arrival counters per sweep buffer
    SweepWork gs_work[2];
    bool small = false;       // n <= 32: fused one-workgroup-per-interval path (dto_small.hip)
    double* d_Gs = nullptr;   // compact generators for that path
    bool use_basis = false;   // A^2..A^4 from the generator subspace instead of three batched GEMMs
    BasisSet basis[3]{};      // degrees 2, 3, 4
    BasisSet basis_all{};     // every multiset of degree 0..4: one GEMM gives the factor K of the two-product Taylor form
    // Hessian pairing path: stored Taylor terms of both sweeps, E_j * forward terms, Beta-weighted adjoint sums
    bool pairing = false;
    double* EP = nullptr;
    double* Upair = nullptr;
    double* d_Btab = nullptr;
    // DTO_FLAG_BLOCK_GENERATORS: G_j = I_r (x) B_j found at create (kb x kb blocks, kr of them; (n, 1) without); `kron`: the
    // structured path (dto_kron.hip) serves the integrator -- none of the workspaces above exist then
    int kb = 0, kr = 1;
    bool kron = false;
    KKron kk{};
    double* d_kron_scratch = nullptr;
    size_t kron_stride = 0;
    // DTO_FLAG_SHARED_GENERATORS: the group of integrators with these generators and controls (indices into dto_handle::bil; the
    // leader is the first member in list order; -1 / 1 without a partner).  `share_active`: the group shares the leader's
    // propagator chain -- a follower runs none, its -E_k blocks are copies of the leader's (dto_share.hip).  `share_followers`
    // (leader of an active group only): the other members in list order.  `list_pos`: position in the integrator list.
    int share_leader = -1, share_size = 1, list_pos = 0;
    bool share_active = false;
    std::vector<int> share_followers;
    bool follows() const { return share_active && share_followers.empty(); }
};

struct ConHost {
    KCon k{};
    int equality = 0;
    int64_t n_times_total = 0;
    int64_t row_off = 0;  // global 0-based first row
    std::vector<int64_t> times0;  // all times (0-based knots), reference order
    std::vector<int32_t> comps;
    int g_dim = 1;
    bool external = false;        // DTO_CONSTRAINT_EXTERNAL[_GLOBAL]: values/Jacobian/Hessian blocks come from dto_set_external
    bool global = false;          // ..._GLOBAL: `comps` index global_data; the single listing sits at the pseudo-knot N
    int ext_slot = -1;
    std::vector<double> jac0;     // external: Jacobian blocks at Z0 (pattern)
    std::vector<double> hess0;    // global: Hessian of sum(g) at Z0 (pattern)
    std::vector<double> M;        // QUADFORM_MINUS_C: the symmetric n_comps x n_comps matrix, column-major
    KExtTerm xk{};                // external: placement of the Hessian blocks
};

// DTO_OBJECTIVE_EXTERNAL_KNOT / _GLOBAL: placement data of a host-evaluated objective term
struct ExtObjHost {
    double weight = 1.0;
    bool global = false;
    std::vector<int32_t> comps, gcomps;
    std::vector<int64_t> times0;  // listed knots, 0-based; {N} for a GlobalObjective (no knot part)
    KExtTerm k{};
    int ext_slot = -1;
};

// one host-evaluated term's values for the coming callbacks + grow-only device staging
struct ExtSlot {
    dto_external_values v{nullptr, nullptr, nullptr};
    size_t len[3] = {0, 0, 0};   // doubles per array (all listed times)
    double* d[3] = {nullptr, nullptr, nullptr};
};

// DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR: evaluated by dto_tdb.hip (1..64 states), dto_tdb_mfma.hip (65..256 states) or, with
// replicated-block generators, dto_tdb_kron.hip (33..512 states) into per-interval blocks, placed like an external integrator
struct TdbHost {
    KTdb k{};
    KExtInt place{};
    double *d_vals = nullptr, *d_jac = nullptr, *d_hess = nullptr, *d_scratch = nullptr;
    size_t stride = 0;
    double* d_jtv = nullptr;   // every device path: staging of the matrix-free J' w, [K][n + p] (option "tdb_matrix_free_products")
    // 65..256 states: zero-padded generators and their transposes, and the scratch slots (= workgroups) of the persistent grid
    bool mfma = false;
    double *d_Bp = nullptr, *d_BpT = nullptr;
    int resident = 0;
    // DTO_FLAG_BLOCK_GENERATORS: every G_j and H_cj is I_r (x) B_q (kb x kb blocks, kr of them; (n, 1) without); `kron`: the
    // structured path (dto_tdb_kron.hip) serves the integrator -- it shares `resident` and the blocks above, whose constant zeros
    // are written once at allocation
    int kb = 0, kr = 1;
    bool kron = false;
    KKron kk{};
    // DTO_FLAG_SHARED_GENERATORS: the group of time-dependent integrators of one system (indices into dto_handle::tdb; the leader is
    // the first member in list order, -1: no partner).  ACTIVE groups (k_tdb_mfma members, two or more) are evaluated by the group
    // form of the kernel, at most `share_cap` members per launch.  Leader only: `share_members` (all of them, itself first) and the
    // group launches' scratch, `resident` slots of `share_stride` doubles.  `list_pos`: position in the integrator list.
    int share_leader = -1, share_size = 1, share_cap = 1, list_pos = 0;
    bool share_active = false;
    std::vector<int> share_members;
    double* d_share_scratch = nullptr;
    size_t share_stride = 0;
};

struct ProfRec {
    hipEvent_t a, b;
    int cat;
    double flops;
};

// ChainWork::smax[0..7] as the host reads it back, member for member as launch_expm_params, launch_expm_coef, launch_norm1_one and
// launch_chain64 write it
struct ChainReadback {
    int32_t s_max2, s_sum2;   // two-product form: largest squaring count and the sum of the counts over the chunk
    double d2max;             // max_k ||A_k^2||_1^(1/2) (smax[2..3])
    int32_t s_max3, s_sum3;   // three-product form
    int32_t form;             // the evaluation form taken (2 or 3)
    int32_t pad;
};
static_assert(sizeof(ChainReadback) == 32 && std::is_standard_layout<ChainReadback>::value, "ChainReadback mirrors eight int32 of ChainWork::smax");

// The handle's pinned host memory: where the asynchronous device-to-host copies of the few scalars the host plans from land, one
// typed member per destination (the copies leave on the call's stream, the sweep's and the readback stream: none overlaps another).
struct PinnedMailbox {
    double bounds[2];              // enqueue_bounds: max beta, max b1
    ChainReadback chain;           // the chain's readback (32 bytes; exact_d2 copies the first 16)
    int32_t sweep_stats[2];        // fused_sweep_steps: a sweep's two statistics; step-per-launch sweeps: their checkpoints, alternating
    unsigned long long hump[8];    // k_hump's output (read_hump)
    int32_t same_flag;             // same_point's bit compare
    int32_t hp_flag;               // the kept points' bit compares (DevicePoint::flag names its member): hess_product's,
    int32_t dyn_flag;              // dynamics_solve's,
    int32_t elim_flag;             // the whole-dynamics solves',
    int32_t red_flag;              // the reduced point's
    int32_t deferred_smax;         // the one-launch chain's squaring count of an enqueue-only call (smax_pending)
    double newton[2];              // the truncated-Newton step's (status, iterations) after every iteration
    double precond[3];             // the preconditioned step's (status, iterations, pairs taken) after every iteration
    double minimize[4];            // the minimize call's (accepted / grew, delta for the next step, stop, phi) after every trial and outer iteration
    double minimize_step[3];       // and the step's (status, iterations, ||g||) in front of a trial's merit: the gradient test
};

struct Workspace { double* p = nullptr; size_t cap = 0; };   // grow-only device buffer, capacity in doubles (grow_workspace, dto_engine.cpp)

// A kept point (dto_kept_point.h states the protocol): the host record, the device copies of the Z and mu it was built at, the bit
// compare's device flag and the mailbox member it comes back into.  The handle owns the memory, whichever allocation it lies in.
struct DevicePoint {
    KeptPoint rec;
    int32_t PinnedMailbox::*flag;
    double *d_Z = nullptr, *d_mu = nullptr;   // d_mu null: mu is no part of the point
    int32_t* d_flag = nullptr;
    DevicePoint(unsigned parts, int32_t PinnedMailbox::*f) : rec(parts), flag(f) {}
};
}  // namespace dto

struct dto_handle {
    std::string err;
    int device = 0;
    bool structure_only = false;  // created with device < 0: sizes, structure and shard queries only
    int64_t N = 0, K = 0;
    int z = 0, gd = 0, dt_idx = 0, D = 0;
    int eval_hessian = 1;
    int64_t n_vars = 0, n_cons = 0, n_dyn = 0, jac_nnz = 0, hess_nnz = 0;
    int64_t k_lo = 1, k_hi = 1;
    dto::KProb P{};
    std::vector<int64_t> colptr;            // host copy
    std::vector<int64_t> con_cols, con_rows;  // constraint pattern entries sorted by (col,row), 0-based
    std::vector<dto::BilHost> bil;
    std::vector<dto::KDer> der;
    std::vector<int> integ_kind, integ_index;  // reference order -> (kind, index into bil/der)
    std::vector<int> integ_dim;
    std::vector<int64_t> integ_row_off;
    std::vector<dto::ConHost> con;
    std::vector<dto::KObj> obj;
    struct ObjInfo {  // host copy of what a built-in objective term touches in the Hessian (the D2H plan needs it)
        int kind, comp_off, comp_dim;
        std::vector<int32_t> comps;
        std::vector<int64_t> times;  // owned, 0-based
        // The term's listings are stored in LAYERS: layer l holds the (l+1)-th listing of every knot, so that inside one layer
        // no two listings name the same knot.  Gradient and Hessian kernels run layer by layer (one launch each; a single
        // layer unless `times` repeats a knot): contributions to one entry are added in listing order, never concurrently.
        std::vector<int64_t> layer_start;  // [n_layers + 1] offsets into the (layer-sorted) listing arrays
    };
    std::vector<ObjInfo> obj_info;
    // host-pointer entry points: only the entries that can change cross PCIe (dto_hostxfer.h); built lazily at the first
    // host-pointer Jacobian / Hessian call, option "host_xfer" = 0 keeps the plain whole-slab copy
    std::unique_ptr<dto::HostXfer> xfer;
    dto::XferPlan jac_plan, hess_plan;
    bool plans_built = false;
    bool raw_plans_built = false;
    // dto_bind_output_dev: a device buffer the caller passes again and again (MadNLP's value vectors in GPU mode).  Once a call
    // has written it in full ("primed"), later calls into the SAME pointer leave the call-invariant entries alone -- structural
    // zeros, the identity z_{k+1} halves: half of a Jacobian slab, 99 % of a Hessian slab -- and clear only the runs a kernel
    // accumulates into.  [0] Jacobian, [1] Hessian.
    double* bound[2] = {nullptr, nullptr};
    bool primed[2] = {false, false};
    int64_t* d_bind_start[2] = {nullptr, nullptr};
    int64_t* d_bind_len[2] = {nullptr, nullptr};
    int64_t n_bind_runs[2] = {0, 0};
    bool bind_ready[2] = {false, false};
    int host_xfer = 1;
    int xfer_check = 0;  // option "host_xfer_check": every host-pointer Jacobian / Hessian is compared with the whole device slab
    std::vector<dto::ExtObjHost> ext_obj;
    std::vector<dto::KExtInt> ext_int;  // DTO_INTEGRATOR_EXTERNAL, slot = index
    std::vector<dto::TdbHost> tdb;      // DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR
    std::vector<dto::ExtSlot> ext;      // external integrators, then constraints, then objectives, each in list order
    int n_ext_int = 0, n_ext_con = 0, n_ext_obj = 0;
    std::vector<int64_t> tail_colptr, tail_rows;  // Hessian entries in global-variable columns (CSC tail)
    int64_t hess_block_nnz = 0;
    std::vector<std::pair<int64_t, int64_t>> row_segments;  // (global start 0-based, len)
    int64_t cons_len = 0;
    dto_shard_info info{};

    // device scratch
    int64_t* d_colptr = nullptr;
    double* d_Z = nullptr;
    double* d_mu = nullptr;
    double* d_out = nullptr;  // host-API staging for the largest output
    size_t d_out_cap = 0;
    double* d_partial = nullptr;
    double* d_f = nullptr;
    double* d_bounds = nullptr;  // [2] max beta, max b1 (as uint64 bit patterns)
    int32_t* d_plan = nullptr;   // [4] {q, d_ub, tc} of a sweep planned on the device from d_bounds (launch_plan_dev)
    double* d_jac_scratch = nullptr;     // value slab for the Jacobian-vector products (lazy)
    double* d_w = nullptr;               // product input
    uint64_t gen = 0;   // the generation every kept point (dto_kept_point.h) is keyed by: drop_caches bumps it
    // open-loop rollout (dto_rollout[_dev]): product tree, padded trajectory and the host-pointer form's X0
    dto::Workspace d_roll_tree, d_roll_S, d_roll_X0;
    // solves with the dynamics block (dto_dynamics_solve[_dev]): their kept point is the product tree in d_roll_tree, tagged with the
    // integrator; a rollout overwrites the tree and drops the point.  The offset tree and the host-pointer form's B.
    dto::Workspace d_dyn_off, d_dyn_B;
    dto::DevicePoint dyn_point{dto::KeptPoint::TAG, &dto::PinnedMailbox::dyn_flag};
    // whole-dynamics solves (dto_dynamics_solve_all[_dev]; plan: dto_elim_plan.h): their kept point is a product tree per integrator
    // (by list position, empty for a DerivativeIntegrator) and the compact coupling store, all the call's own: neither dto_rollout nor
    // dto_dynamics_solve touches them.  Bp / Yp: one block solve's right-hand side and result; d_elim_B: the host-pointer form's B.
    std::unique_ptr<dto::ElimPlan> elim;
    std::vector<dto::Workspace> elim_tree;
    dto::KElimTerm* d_elim_terms = nullptr;          // forward terms of every integrator, then the adjoint terms
    std::vector<int> elim_fw_term0, elim_ad_term0;   // [I + 1] ranges in d_elim_terms
    dto::Workspace d_elim_store, d_elim_Bp, d_elim_Yp, d_elim_B;
    dto::DevicePoint elim_point{0, &dto::PinnedMailbox::elim_flag};
    // reduced-space operators (dto_reduced_gradient[_dev], dto_reduced_hessian_product[_dev]; plan: dto_reduced_plan.h).  One block
    // d_red holds every vector; its sizes depend on the handle alone, so it is allocated once, before anything is enqueued, and freed
    // with the handle.  The reduced POINT -- keyed by sigma and the mark "mu was NULL" too, its copies of Z and mu inside d_red -- holds
    // g (red_g), the costates Lam [N][D] (red_lam), the multipliers mu~ (red_mut) and the reduced gradient (red_r).  a, b [n_vars],
    // w [n_cons], s1, s2 [N D]: scratch of one call; hv, hmu: v and mu of the host-pointer forms; out: their y.
    dto::KReduced red{};   // device tables
    double* d_red = nullptr;
    double *red_g = nullptr, *red_lam = nullptr, *red_mut = nullptr, *red_r = nullptr;
    double *red_a = nullptr, *red_b = nullptr, *red_w = nullptr, *red_s1 = nullptr, *red_s2 = nullptr;
    double *red_hv = nullptr, *red_hmu = nullptr, *red_out = nullptr;
    dto::DevicePoint red_point{dto::KeptPoint::SIGMA | dto::KeptPoint::MU_MARK, &dto::PinnedMailbox::red_flag};
    // the operators' input-block store (option "reduced_input_store"; plan: dto_input_plan.h): the tables once per handle, the store
    // F grow-only and kept with the whole-dynamics solves' point (elim_point: gathered in the same rebuild, from the same slab)
    int reduced_input_store = 0;   // option of that name: 1 takes J v^ and J' w of the reduced operators from the kept input blocks
    std::unique_ptr<dto::InputPlan> input;
    dto::KInput in{};              // device tables
    dto::Workspace d_in_store;
    // block products (dto_eval_hessian_products[_dev], dto_projected_hessian_products[_dev]): option "reduced_block_width" caps the
    // columns per chunk (0: the engine's choice).  d_blk: one chunk's B, Y [N][W][D], z^ and q [W][n_vars] and, off the store route,
    // rho / w [W][n_cons]; d_blk_host: the host-pointer forms' V and Y.  Both grow-only, sized before anything is enqueued.
    int reduced_block_width = 0;
    dto::Workspace d_blk, d_blk_host;
    // feasible-trajectory rollout and reduced merit value (dto_feasible_trajectory[_dev], dto_feasible_merit[_dev]; schedule:
    // dto_feasible_plan.h).  The rollout works in the caller's Zf and in dto_rollout's tree and trajectory workspaces.  d_feas, the
    // merit's own block, grow-only and sized before anything is enqueued: Zf [n_vars] and g [n_cons] where the caller gives none, the
    // host-pointer form's mu [n_cons], f and phi.
    std::unique_ptr<dto::FeasiblePlan> feas;
    dto::Workspace d_feas;
    // truncated-Newton step (dto_projected_newton_step[_dev]; dto_newton_plan.h, dto_newton.hip).  d_newton: r, d and y / w [n_vars], the
    // partial sums [8][chunks] and the scalars [16]; d_newton_host: the host-pointer form's mask and p [n_vars], info [8] and trace
    // [max_iter][4].  Both grow-only, sized before anything is enqueued.  The products run in d_blk (one column).
    dto::Workspace d_newton, d_newton_host;
    // bound-constrained step (dto_projected_newton_step_box[_dev]; dto_newton_box_plan.h, dto_newton_box.hip).  d_newton_box: r, d and
    // y / w [n_vars], the partial results [12][chunks], the scalars [16] and the state bytes [n_vars]; d_newton_box_host: the
    // host-pointer form's mask, lo, hi, p, Zp and entry_state [n_vars] each, info [12] and trace [max_iter][6].  Grow-only like the above.
    dto::Workspace d_newton_box, d_newton_box_host;
    // L-BFGS-preconditioned step (dto_preconditioned_newton_step[_dev], dto_newton_precondition[_dev], dto_newton_pairs_*;
    // dto_precond_plan.h, dto_precond.hip).  newton_pairs: the option of that name, the store's capacity m (0: off).  d_pairs: the
    // store, two banks of 2 m vectors [n_vars] (allocated whole by the first push or harvest; setting the option clears it);
    // pairs_bank the current bank, in which pairs_count pairs lie as a ring from slot pairs_head.  d_precond: the routine's workspace
    // (precond_workspace_doubles); d_precond_host: the host-pointer forms' vectors.
    int newton_pairs = 0, pairs_bank = 0, pairs_count = 0, pairs_head = 0;
    dto::Workspace d_pairs, d_precond, d_precond_host;
    // reduced-space minimize (dto_projected_minimize[_dev]; dto_minimize_plan.h, dto_minimize.hip).  d_minimize: p, Zp, Zt [n_vars] each,
    // the step's info [16], the two banks of scalars [16] each, the two row passes' scalars [8] each, phi_t and the mailbox [4];
    // d_minimize_host: the host-pointer form's Z, mask, lo, hi, entry_state [n_vars] each, mu, rho [n_cons] each, info [16] and the
    // two histories.  Grow-only like the above.
    dto::Workspace d_minimize, d_minimize_host;
    // augmented-Lagrangian terms (dto_auglag_*; dto_auglag_plan.h, dto_auglag.hip).  d_al: mu_eff, weight, g, the rows of the
    // single-column route and the host-pointer forms' mu and rho [n_cons] each, then info [8]; d_al_t: the planes t [W][n_vars] of the
    // Gauss-Newton term; d_al_host: the host-pointer forms' lam [N n_states].  d_al_eq: the equality flag of every non-dynamics row,
    // one byte each, written once.  Grow-only like the above.
    dto::Workspace d_al, d_al_t, d_al_host;
    unsigned char* d_al_eq = nullptr;
    int64_t* d_conbase = nullptr;       // [n_vars+1] first constraint-pattern entry of each column
    int64_t* d_crow_ptr = nullptr;       // the constraint pattern in row order (J w gathers rows): [rows+1], columns, slab positions
    int64_t* d_crow_col = nullptr;
    int64_t* d_crow_pos = nullptr;
    int64_t* d_con_rows = nullptr;       // constraint-pattern rows, (col,row) order
    dto::PinnedMailbox* mailbox = nullptr;  // pinned; every readback the host plans from lands in a member of its own
    bool smax_pending = false;   // the one-launch chain's squaring count lands in mailbox->deferred_smax behind ev_done (read by check_sweeps)
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // generator sweep runs here, concurrently with the propagator chain
    hipStream_t stream_rb = nullptr; // the chain's 96-byte readback (evaluation form, squaring counts, hump bound) leaves on this one
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_stats = nullptr, ev_chain = nullptr, ev_rb = nullptr, ev_zero = nullptr;

    bool reuse = false;          // option reuse_forward_sweep
    double* d_Zcache = nullptr;  // the Z the cached sweeps belong to
    int32_t* d_eq = nullptr;
    bool profiling = false;
    std::vector<dto::ProfRec> prof;
    int64_t sweep_forms[5] = {0, 0, 0, 0, 0};  // run_sweep calls by the form they took (SWEEP_GS ..), counted while profiling
    std::vector<hipEvent_t> ev_pool;  // recycled timing events (creating them inside the timed region costs host time)
    int last_smax = 0, last_terms = 0;
    int expm_form = 0;  // option "expm_form": 0 = by cost, 2 / 3 = forced
    int overlap_sweep = 1;  // option "overlap_sweep": the Jacobian's generator sweep on a second stream next to the chain's products
    int sweep_form = 0;   // option "sweep_form": 0 = fused persistent sweep where it applies, 1 = step-per-launch form only
    int chain_form = 0;   // option "chain_form": 0 = the one-launch chain of 33..64-state integrators where it applies, 1 = batched-GEMM launches only
    int n_cu = 256;
    int chain_chunk = 0;  // option "chain_chunk": upper bound on the intervals per chain chunk (0: workspace capacity)
    int tdb_share_members = 0;  // option of that name: members per group launch of k_tdb_mfma (0: each group's cap from create)
    int tdb_resident = 0;  // option of that name: cap on the persistent grid of k_tdb_mfma / k_tdb_kron launches, product forms included (0: each integrator's `resident`)
    int tdb_matrix_free_products = 0;  // option of that name: J w / J' w of device time-dependent integrators (dense or structured) without a slab
    int deterministic = 0;  // option "deterministic": results independent of overlap_sweep and of the entry-point family
    // deferred errors of the `*_dev` entry points (dto_engine.h, error convention): the sweep statistics of the last
    // asynchronous call are copied to pinned memory behind its kernels and looked at by the next call through the ABI
    hipEvent_t ev_done = nullptr;
    bool stats_pending = false;
    int32_t* h_stats = nullptr;  // pinned [2 * bilinear integrators][2]
    int last_form = 0;
    // multi-GPU (dto_comm.h): the knot ranges of the communicator's ranks (dto_comm_create exchanges them over RCCL,
    // dto_comm_set_ranges takes them from a caller with a transport of its own), the gather plans that follow from them,
    // and the communicator itself
    std::unique_ptr<dto::Comm> comm;
    int comm_rank = -1;
    std::vector<std::pair<int64_t, int64_t>> rank_ranges;               // (k_lo, k_hi) per rank, 1-based inclusive
    dto::GatherPlan gather_plan[4];                                           // DTO_VECTOR_* - 1
    std::vector<dto::Slab> cons_segments;                                     // every rank's row segments of g ...
    std::vector<int> cons_segment_root;                                  // ... and the rank that owns each
    int64_t* d_ranges = nullptr;
    // Hessian-vector products (dto_eval_hessian_product[_dev]): H is assembled once per point into a private slab, its entries
    // that can be non-zero are gathered into a row-major copy of both triangles, and every product at that point is one launch
    // (dto_hess_product.hip).  The kept point is keyed by sigma and always holds a mu.
    double* hp_slab = nullptr;       // [hess_len], allocated at the first product
    bool hp_slab_primed = false;     // written in full once: later points clear only the variable runs (as a bound output)
    bool hp_index = false;
    dto::KHessProduct hp{};
    int64_t hp_nnz = 0;              // entries of the row-major copy (odd rows padded)
    int64_t* d_hp_pos = nullptr;     // [hp_nnz] slab position of every entry, -1 for padding
    double* d_hp_val = nullptr;
    double* d_hp_v = nullptr;        // host-pointer form: v
    dto::DevicePoint hp_point{dto::KeptPoint::SIGMA, &dto::PinnedMailbox::hp_flag};
    double hp_setup_ms = 0.0;        // host time of the index build ...
    double hp_bytes = 0.0;           // ... and the device bytes of the private slab and the index
    std::vector<void*> owned;  // device allocations to free

    ~dto_handle();
};

namespace dto {

template <class T>
T* own(dto_handle* h, T* p) {
    h->owned.push_back(p);
    return p;
}

inline int fail(dto_handle* h, const std::string& m) {
    if (h) h->err = m; else g_create_error = m;
    return 1;
}

inline int pad64(int n) { return ((n + 63) / 64) * 64; }

// the dimensions every position in the two value slabs follows from (dto_slab_layout.h states the layout)
inline SlabDims slab_dims(const dto_handle* h) { return SlabDims{h->N, h->K, (int32_t)h->z, (int32_t)h->D}; }

// first constraint-pattern entry of column c
inline size_t con_lower(const dto_handle* h, int64_t c) {
    return std::lower_bound(h->con_cols.begin(), h->con_cols.end(), c) - h->con_cols.begin();
}

// position in this handle's Jacobian slab of the i-th constraint-pattern entry of column col
inline int64_t con_entry_pos(const dto_handle* h, int64_t col, int64_t i) {
    return h->colptr[col] + jac_con_off(slab_dims(h), col / h->z) + i - h->P.jac_lo;
}

// value slabs of the handle that owns knots k_lo..k_hi (1-based, inclusive): positions inside the global vectors
struct ShardExtents {
    int64_t grad_lo, grad_len, jac_lo, jac_len, hess_lo, hess_len;
};
ShardExtents shard_extents(const dto_handle* h, int64_t k_lo, int64_t k_hi);

// rows of g that handle owns, as (global 0-based start, length) segments in the order of its local buffer: per integrator the
// rows of the owned intervals, then per constraint the listed times at owned knots (runs of consecutive listings merged)
std::vector<std::pair<int64_t, int64_t>> shard_row_segments(const dto_handle* h, int64_t k_lo, int64_t k_hi);

}  // namespace dto
