// dto_engine.cpp -- evaluation side of the C ABI declared in include/dto_engine.h.
//
// Orchestrates the HIP kernels of dto_kernels.hip on a handle (dto_handle.h) that dto_create.cpp built: sweep planning, the
// propagator chain, the callbacks, the transfer plans, the extern "C" entry points other than dto_create, the communicator and
// profiling.  There is NO CPU fallback: every evaluation runs on the GPU or fails with an error code.
#include "dto_handle.h"
#include "dto_auglag_plan.h"
#include "dto_newton_box_plan.h"
#include "dto_minimize_plan.h"
#include "dto_precond_plan.h"
#include "dto_newton_plan.h"
#include "dto_rollout_plan.h"

#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <map>

using namespace dto;

thread_local std::string dto::g_create_error;

dto_handle::~dto_handle() {
    if (structure_only) return;
    (void)hipSetDevice(device);
    comm.reset();
    for (auto& r : prof) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    for (auto& e : ev_pool) (void)hipEventDestroy(e);
    for (void* p : owned) (void)hipFree(p);
    if (mailbox) (void)hipHostFree(mailbox);
    if (stream) (void)hipStreamDestroy(stream);
    if (stream2) (void)hipStreamDestroy(stream2);
    if (stream_rb) (void)hipStreamDestroy(stream_rb);
    if (ev_rb) (void)hipEventDestroy(ev_rb);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_zero) (void)hipEventDestroy(ev_zero);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (ev_stats) (void)hipEventDestroy(ev_stats);
    if (ev_chain) (void)hipEventDestroy(ev_chain);
    if (ev_done) (void)hipEventDestroy(ev_done);
    if (h_stats) (void)hipHostFree(h_stats);
}

namespace {

struct ProfScope {
    dto_handle* h;
    hipStream_t st;
    bool on;
    ProfRec r{};
    ProfScope(dto_handle* h_, hipStream_t st_, int cat, double flops) : h(h_), st(st_), on(h_->profiling) {
        if (!on) return;
        r.cat = cat;
        r.flops = flops;
        auto take = [&](hipEvent_t& e) {
            if (h->ev_pool.empty()) (void)hipEventCreate(&e);
            else { e = h->ev_pool.back(); h->ev_pool.pop_back(); }
        };
        take(r.a);
        take(r.b);
        (void)hipEventRecord(r.a, st);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(r.b, st);
        h->prof.push_back(r);
    }
};
// (for the bandwidth-bound categories from CAT_ZERO on, `flops` carries the launch's algorithmic BYTES)
// CAT_JAC_PRODUCT ("jac_product"): the J w / J' w launches of the structured and small paths, priced in FLOPS as kron_eval prices a
// sweep -- sixteen terms of 2 b^2 per column and (on average two) sources over the mode's (m + 2) column groups -- so it is part of
// the third output of "all"
enum { CAT_BGEMM = 0, CAT_SWEEP = 1, CAT_OTHER = 2, CAT_BGEMM_HORNER = 3, CAT_BGEMM_SQUARE = 4, CAT_SWEEP_ADJOINT = 5,
       CAT_ZERO = 6, CAT_BUILD_A = 7, CAT_ASSEMBLY = 8, CAT_BASIS_MULTI = 9, CAT_CHAIN64 = 10, CAT_HESS_PRODUCT = 11, CAT_SHARE = 12, CAT_TDB_MFMA = 13, CAT_JAC_PRODUCT = 14, CAT_TDB_KRON = 15, CAT_TDB_PRODUCT = 16, CAT_ROLLOUT = 17, CAT_ROLLOUT_TREE = 18, CAT_ROLLOUT_DESCENT = 19, CAT_DYNSOLVE_TREE = 20, CAT_DYNSOLVE_SCAN = 21, CAT_DYNSOLVE_COUPLE = 22, CAT_DYNSOLVE_DERIV = 23, CAT_REDUCED_PACK = 24, CAT_REDUCED_INPUT = 25, CAT_FEASIBLE = 26, CAT_NEWTON = 27, CAT_NEWTON_BOX = 28, CAT_AUGLAG = 29, CAT_PRECOND = 30, CAT_MINIMIZE = 31 };
// CAT_ROLLOUT .. CAT_ROLLOUT_DESCENT ("rollout" = its parts "rollout_gather" + "rollout_tree" + "rollout_descent"): the gather, the
// tree's products and the descent (with the start and the copy into the caller's layout) of dto_rollout[_dev], flops as executed with
// padding; the tree's products run launch_bgemm_plain and count HERE, not under "bgemm_plain"; they feed no other name, "all" included
inline bool is_rollout_cat(int cat) { return cat >= CAT_ROLLOUT && cat <= CAT_ROLLOUT_DESCENT; }
// CAT_DYNSOLVE_TREE, CAT_DYNSOLVE_SCAN ("dynsolve" = "dynsolve_tree" + "dynsolve_scan"): of dto_dynamics_solve[_dev], the gather and
// the tree's products of a rebuild, and the loader, the offsets' up-sweep, the descent and the copy into the caller's layout; flops as
// executed with padding.  Like the rollout's they feed no other name, "all" included.
inline bool is_dynsolve_cat(int cat) { return cat == CAT_DYNSOLVE_TREE || cat == CAT_DYNSOLVE_SCAN; }
// CAT_DYNSOLVE_COUPLE ("dynsolve_couple"), CAT_DYNSOLVE_DERIV ("dynsolve_deriv"): of dto_dynamics_solve_all[_dev], the gather of the
// coupling blocks with the contractions against them, and the DerivativeIntegrators' block solves; the third output carries BYTES as
// executed.  (Its other block solves count under "dynsolve_tree" / "dynsolve_scan".)  They feed no other name, "all" included.
inline bool is_elim_cat(int cat) { return cat == CAT_DYNSOLVE_COUPLE || cat == CAT_DYNSOLVE_DERIV; }
// CAT_REDUCED_PACK ("reduced_pack"): the packers of dto_reduced_gradient / dto_reduced_hessian_product and their _dev forms
// (dto_reduced.hip); the third output carries BYTES as executed.  It feeds no other name, "all" included; the routines the operators
// are made of count under their own names.
// CAT_REDUCED_INPUT ("reduced_input"): with the option "reduced_input_store", the gather of the input blocks and the two products with
// them (dto_reduced.hip); BYTES as executed; it feeds no other name either.
// CAT_FEASIBLE ("feasible"): the three kernels of dto_feasible.hip -- the DerivativeIntegrators' recurrences, the scatters of the rolled-out
// states and the merit sum of dto_feasible_trajectory / dto_feasible_merit and their _dev forms; BYTES as executed; it feeds no other
// name, "all" included.  The Jacobian, tree and descent launches inside count under their own names.
// CAT_NEWTON ("newton"): the four kernels of dto_newton.hip -- the start, the curvature pass, the step and the direction update of
// dto_projected_newton_step and its _dev form; BYTES as executed; it feeds no other name, "all" included.  The products of the
// iterations count under the names of the block products.
// CAT_NEWTON_BOX ("newton_box"): the four kernels of dto_newton_box.hip, of dto_projected_newton_step_box and its _dev form, likewise.
// CAT_AUGLAG ("auglag"): the kernels of dto_auglag.hip -- the row pass, the Gauss-Newton term, the scaling and the addition of the
// dto_auglag_* calls; BYTES as executed; it feeds no other name, "all" included.
// CAT_PRECOND ("precond"): every launch of dto_preconditioned_newton_step, dto_newton_precondition and dto_newton_pairs_push_dev that is
// no product -- the kernels of dto_precond.hip and the box step's start and curvature pass where the preconditioned step runs them;
// BYTES as executed; it feeds no other name, "all" included.
// CAT_MINIMIZE ("minimize"): the two kernels of dto_minimize.hip, one launch per trial and one per outer iteration of
// dto_projected_minimize and its _dev form; BYTES, a trial's as if it is accepted; it feeds no other name, "all" included.
// The block products (dto_eval_hessian_products, dto_projected_hessian_products) count under the same names -- "hess_product",
// "reduced_pack", "reduced_input" -- one launch per chunk each, bytes as executed: the matrices once per tile or chunk, the vectors per column.
// the form a generator sweep took (SWEEP_GS .. SWEEP_STEP, dto_sweep_plan.h): one count per run_sweep call, not per launch
inline void count_sweep_form(dto_handle* h, int form) {
    if (h->profiling) ++h->sweep_forms[form];
}

}  // namespace

// ------------------------------------------------------------------------------------------
// structure
// ------------------------------------------------------------------------------------------

namespace dto {

// value slabs of the handle that owns knots k_lo..k_hi (1-based, inclusive): positions inside the global vectors
ShardExtents shard_extents(const dto_handle* h, int64_t k_lo, int64_t k_hi) {
    const int64_t kn_lo = k_lo - 1, n_knots = k_hi - k_lo + 1;
    const int64_t c_lo = kn_lo * h->z, c_hi = (kn_lo + n_knots) * h->z;
    const bool last = k_hi == h->N;  // global-variable columns and the Hessian's tail ride with the last knot
    ShardExtents e;
    e.grad_lo = c_lo;
    e.grad_len = c_hi - c_lo + (last ? h->gd : 0);
    e.jac_lo = h->colptr[c_lo];
    e.jac_len = h->colptr[last ? h->n_vars : c_hi] - e.jac_lo;
    e.hess_lo = hess_block_start(slab_dims(h), kn_lo);
    e.hess_len = hess_block_start(slab_dims(h), kn_lo + n_knots) - e.hess_lo + (last ? (int64_t)h->tail_rows.size() : 0);
    return e;
}

// rows of g that handle owns, as (global 0-based start, length) segments in the order of its local buffer: per integrator the
// rows of the owned intervals, then per constraint the listed times at owned knots (runs of consecutive listings merged)
std::vector<std::pair<int64_t, int64_t>> shard_row_segments(const dto_handle* h, int64_t k_lo, int64_t k_hi) {
    const int64_t kn_lo = k_lo - 1, n_knots = k_hi - k_lo + 1;
    const int64_t n_int = std::max<int64_t>(0, std::min<int64_t>(k_hi, h->K) - k_lo + 1);
    std::vector<std::pair<int64_t, int64_t>> seg;
    for (size_t i = 0; i < h->integ_kind.size(); ++i)
        if (n_int > 0) seg.emplace_back(h->integ_row_off[i] + kn_lo * h->integ_dim[i], n_int * h->integ_dim[i]);
    for (auto& c : h->con) {
        int64_t prev = -2;  // index of the previous owned listing of THIS constraint
        for (int64_t i = 0; i < c.n_times_total; ++i) {
            const int64_t kn = c.times0[i];
            if (kn >= h->N ? k_hi != h->N : (kn < kn_lo || kn >= kn_lo + n_knots)) continue;  // pseudo-knot N: last rank
            if (!seg.empty() && prev == i - 1 && seg.back().first + seg.back().second == c.row_off + i * c.g_dim)
                seg.back().second += c.g_dim;
            else
                seg.emplace_back(c.row_off + i * c.g_dim, c.g_dim);
            prev = i;
        }
    }
    return seg;
}

}  // namespace dto

namespace {

// ------------------------------------------------------------------------------------------
// sweeps and chain
// ------------------------------------------------------------------------------------------

// Step budget, launch shapes and the form a sweep takes: dto_sweep_plan.h (plain C++, testable without a GPU).  What stays here
// enqueues work or reads the handle.

struct Bounds {
    double beta, b1;
};
Bounds read_bounds(const dto_handle* h) { return Bounds{h->mailbox->bounds[0], h->mailbox->bounds[1]}; }

// enqueue only: the two doubles land in mailbox->bounds in stream order (read them after a later synchronisation point)
void enqueue_bounds(dto_handle* h, BilHost& b, const double* dZ, hipStream_t st) {
    HIP_CHECK(hipMemsetAsync(h->d_bounds, 0, 2 * sizeof(double), st));
    launch_norm_bounds(st, h->P, b.k, dZ, b.d_g1, b.d_n2, reinterpret_cast<unsigned long long*>(h->d_bounds));
    HIP_CHECK(hipMemcpyAsync(h->mailbox->bounds, h->d_bounds, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
}
Bounds get_bounds(dto_handle* h, BilHost& b, const double* dZ, hipStream_t st) {
    enqueue_bounds(h, b, dZ, st);
    HIP_CHECK(hipStreamSynchronize(st));
    return read_bounds(h);
}

void read_hump(dto_handle* h, BilHost& b);
SweepPlan plan_hump(const BilHost& b, double beta_fallback);
SweepPlan plan_sweep(double beta) { return dto::plan_sweep(beta, sweep_theta_v()); }
bool cheap_plan(const Bounds& bd, bool loose, SweepPlan& out) { return dto::cheap_plan(bd.beta, loose, sweep_theta_v(), out); }

// Taylor steps a fused sweep (already enqueued on st) actually took: waits for it.
int fused_sweep_steps(dto_handle* h, const SweepBuf& w, int d_ub, hipStream_t st) {
    int32_t* hs = h->mailbox->sweep_stats;
    HIP_CHECK(hipMemcpyAsync(hs, w.stats, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return std::max(1, std::min(hs[1] - 1, d_ub));
}
bool ensure_bind_runs(dto_handle* h, int which);

// The form a sweep takes: choose_sweep(const SweepSituation&) of dto_sweep_plan.h, asked with what the handle, the integrator, the
// sweep's buffers and the plan say
SweepChoice choose_sweep(const dto_handle* h, const BilHost& b, const SweepBuf& w, const SweepTypes& ty, const SweepPlan& plan,
                         bool store, bool shared_chip, bool step_only = false) {
    return dto::choose_sweep(SweepSituation{w.npad, w.Kpad, b.k.m, ty, h->P.n_int, h->n_cu, h->sweep_form, h->reuse, /*frozen=*/w.frozen != nullptr,
                                            /*has_term_store=*/w.Zt != nullptr, w.dcap, plan.q, plan.d_ub, store, shared_chip, step_only});
}

// Does this sweep run in the 64-state generator-stationary form, which can read its step budget from device memory?  (No term
// store, no reuse: the host then needs nothing of the plan.)  `alone`: the choice of such a sweep with the chip to itself.
const SweepPlan PLAN_ON_DEVICE{1, 200};  // what the host passes where launch_plan_dev's {q, d_ub, tc} are read instead
bool s64_plans_itself(const dto_handle* h, const BilHost& b, const SweepBuf& w, const SweepTypes& ty, SweepChoice* alone = nullptr) {
    if (h->reuse) return false;
    const SweepChoice c = choose_sweep(h, b, w, ty, PLAN_ON_DEVICE, /*store=*/false, /*shared_chip=*/false);
    if (alone) *alone = c;
    return c.form == SWEEP_S64;
}

// 33..64 states: the propagator chain as one launch (dto_chain64.hip)
bool chain64_applies(const dto_handle* h, const BilHost& b) {
    static const int chain64_on = tune_int("DTO_CHAIN64", 1);  // A/B runs (TUNING builds)
    return b.k.npad == 64 && chain64_on && h->chain_form != 1 && h->P.n_int <= b.chain_cap;
}

SweepWork& ensure_sweep_work(dto_handle* h, SweepWork& k, size_t doubles, int counters, size_t counters_alloc) {
    if (doubles > k.cap || counters > k.counters)
        k = SweepWork{own(h, dalloc<double>(doubles)), own(h, dalloc<unsigned>(counters_alloc)), doubles, counters};
    return k;
}

// What run_sweep takes besides the buffers, the plan and the stream, set by name: SweepArgs().keep_terms(keep) ...
struct SweepArgs {
    int src_kind = 0, transposed = 0;  // forward sweep from the states x_k; adjoint(): transposed, from the multipliers mu_k
    bool store = false;        // keep every term in w.Zt (term t of all types at Zt + t*T*Kpad*npad) instead of ping-ponging two buffers
    bool want_steps = false;   // one-launch forms: wait for the sweep and return the steps it took instead of the budget
    bool shared_chip = false, step_only = false;   // see choose_sweep
    int prof_cat = CAT_SWEEP;
    const int32_t* plan_dev = nullptr;    // {q, d_ub, tc} in device memory (launch_plan_dev): the single-workgroup forms only
    const SweepChoice* choice = nullptr;  // choose_sweep's answer from a caller that asked first; else run_sweep asks
    SweepArgs& adjoint(int cat) { src_kind = transposed = 1; prof_cat = cat; return *this; }
    SweepArgs& keep_terms(bool v) { store = v; return *this; }
    SweepArgs& wait_for_steps(bool v) { want_steps = v; return *this; }
    SweepArgs& beside_others(bool v) { shared_chip = v; return *this; }
    SweepArgs& initialised() { step_only = true; return *this; }
    SweepArgs& planned_on_device(const int32_t* p) { plan_dev = p; return *this; }
    SweepArgs& as_chosen(const SweepChoice& c) { choice = &c; store = c.store; shared_chip = c.shared_chip; return *this; }
};

// Returns the number of Taylor steps enqueued in the last round.
int run_sweep(dto_handle* h, BilHost& b, SweepBuf& w, const SweepTypes& ty, const double* dZ, const double* dmu,
              const SweepPlan& plan, hipStream_t st, const SweepArgs& a = SweepArgs{}) {
    const SweepChoice c = a.choice ? *a.choice : choose_sweep(h, b, w, ty, plan, a.store, a.shared_chip, a.step_only);
    if (a.plan_dev && !c.one_workgroup()) throw HipError{"run_sweep: a device-side plan without the form that reads it"};
    const double flops_step = [&] {
        double segs = 0;
        for (int t = w.frozen ? w.first_type : 0; t < ty.T; ++t) segs += b.k.m + 1;  // an extra term rides in the segment of its generator
        return 2.0 * b.k.npad * (double)b.k.npad * w.Kpad * segs;
    }();
    const int tc = sweep_tc(plan);   // first step of the termination test
    count_sweep_form(h, c.form);
    if (c.form != SWEEP_STEP) {
        // the one-launch forms: the whole series, termination tests included, in one persistent launch
        const int wi = &w == &b.ad ? 1 : 0;
        w.nblk = c.form == SWEEP_GS ? c.gs.ipw : c.form == SWEEP_CLUSTER ? c.cluster.ipw : c.fused.ipw;
        SweepWork* k = nullptr;
        if (c.form == SWEEP_GS)   // (the launch zeroes its counters four at a time)
            k = &ensure_sweep_work(h, b.gs_work[wi], sweep_gs_norm_doubles(c.gs), c.gs.n_groups, (size_t)(c.gs.n_groups + 3) / 4 * 4);
        if (c.form == SWEEP_CLUSTER)
            k = &ensure_sweep_work(h, b.cluster_work[wi], sweep_cluster_workspace_doubles(w.npad, c.cluster), c.cluster.n_clusters,
                                   (size_t)c.cluster.n_clusters);
        HIP_CHECK(hipMemsetAsync(w.stats, 0, 4 * sizeof(int32_t), st));
        {
            // flops of the step budget (an upper bound: workgroups leave when their columns have converged)
            ProfScope ps(h, st, a.prof_cat, flops_step * plan.d_ub * plan.q);
            if (c.form == SWEEP_GS)   // (q == 1)
                HIP_CHECK(launch_sweep_gs(st, h->P, b.k, w, ty, c.gs, k->slab, k->arrive, dZ, dmu, a.src_kind, a.transposed, plan.d_ub, tc,
                                          a.store, 1.1e-16));
            else if (c.form == SWEEP_CLUSTER)
                HIP_CHECK(launch_sweep_cluster(st, h->P, b.k, w, ty, c.cluster, k->slab, k->arrive, dZ, dmu, a.src_kind, a.transposed, plan.q,
                                               plan.d_ub, tc, a.store, 1.1e-16));
            else
                HIP_CHECK(launch_sweep_fused(st, h->P, b.k, w, ty, c.fused, dZ, dmu, a.src_kind, a.transposed, plan.q, plan.d_ub, tc, a.store,
                                             1.1e-16, a.plan_dev));
        }
        return a.want_steps ? fused_sweep_steps(h, w, plan.d_ub, st) : plan.d_ub;
    }
    w.nblk = w.TN;
    const size_t tstride = (size_t)ty.T * w.Kpad * w.npad;
    SweepBuf ws = w;
    if (a.store) ws.Z[0] = w.Zt;
    if (w.frozen) launch_sweep_init_tangents(st, ws, ty.T);  // scale factors and type-0 sums are those of the earlier callback
    else if (!a.step_only) launch_sweep_init(st, h->P, b.k, ws, ty, dZ, dmu, a.src_kind, plan.q);
    int launched = 0;
    // one timed region per sweep (steps, termination tests and the gaps between them): an event pair per step costs
    // 0.2 ms per Jacobian call at 256x2000.  Its flop count covers every enqueued step, including the few that find their
    // column blocks already converged (bench.py prices the sweep by the terms actually used, dto_last_stats).
    ProfScope ps(h, st, a.prof_cat, 0.0);
    for (int round = 0; round < plan.q; ++round) {
        if (round > 0) launch_sweep_restart(st, w, ty.T);
        int buf = 0;
        launched = 0;
        bool pending = false;
        int slot = 0;
        // (each termination test left out before tc is one kernel and one dependent-launch gap less, ~12 us; the term-norm
        // slots the tests recycle are cleared once instead)
        for (int t = 0; t < plan.d_ub; ++t) {
            if (tc > 0 && t == tc - 1)
                HIP_CHECK(hipMemsetAsync(w.termnorm, 0, sizeof(unsigned long long) * (size_t)3 * w.T_alloc * w.Kpad, st));
            {
                ps.r.flops += flops_step;
                if (a.store) {
                    ws.Z[0] = w.Zt + (size_t)t * tstride;
                    ws.Z[1] = w.Zt + (size_t)(t + 1) * tstride;
                    // one stored type: split K over the generators, the next terms' slots are the scratch
                    const bool split = ty.T == 1 && (int64_t)(t + b.k.m + 4) <= (int64_t)w.dcap * (1 + b.k.m);
                    launch_sweep_step(st, b.k, ws, ty, a.transposed, t, 0, split ? 1 : 0);
                } else {
                    launch_sweep_step(st, b.k, w, ty, a.transposed, t, buf);
                }
            }
            if (t >= tc) launch_sweep_check(st, w, ty.T, t, 1.1e-16);
            buf ^= 1;
            launched = t + 1;
            // Every 4 steps the number of still-active column blocks (4 bytes) is copied back; the copy of the
            // PREVIOUS checkpoint is read before enqueueing more, so the host never waits on the GPU's current
            // work (the decision lags by 4 steps, which then cost ~5 us each as inactive blocks exit at once).
            if (t >= 3 && (t % 4) == 3 && t + 1 < plan.d_ub) {
                int32_t* hs = h->mailbox->sweep_stats;
                if (pending) {
                    HIP_CHECK(hipEventSynchronize(h->ev_stats));
                    if (hs[slot ^ 1] == 0) break;
                }
                HIP_CHECK(hipMemcpyAsync(hs + slot, w.stats, sizeof(int32_t), hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipEventRecord(h->ev_stats, st));
                pending = true;
                slot ^= 1;
            }
        }
    }
    return launched;
}

// What a caller of the chain asks for per chunk of intervals: a cap on the chunk (0: none; ignored under option "deterministic")
// and `done(first local interval, count)`, run on the host when the -E_k of a chunk are final behind what is enqueued.
struct ChainChunks {
    int cap = 0;
    std::function<void(int64_t, int)> done;
};

// Everything one call of run_chain takes from its caller; every callback may be empty.
struct ChainCall {
    ChainChunks chunks;
    // runs on the host while the GPU works on the first chunk's factor K (one-launch chain: on the launch itself) and the host
    // would otherwise only wait for the readback: independent work to enqueue
    std::function<void()> in_bubble;
    // `after_last_enqueue(d2max)` runs on the host once every kernel of the chain has been enqueued (the GPU is then busy with
    // the Taylor products and squarings): the caller uses it to drive the generator sweep on a second stream so that both
    // proceed concurrently.  d2max = max_k ||A_k^2||_1^(1/2) (exact) bounds the growth of the Taylor terms of the sweep.
    std::function<void(double)> after_last_enqueue;
    bool nothing_waits = false;   // one-launch chain: the caller's sweep is planned and enqueued, the host reads nothing back
};

// exp(dt G(u_k)) for every owned interval; -E_k goes straight into the Jacobian slab.
void run_chain(dto_handle* h, BilHost& b, const double* dZ, double* vals, hipStream_t st, const ChainCall& call) {
    const int npad = b.k.npad;
    const int64_t nint = h->P.n_int;
    double d2max = 0.0;
    if (nint <= 0) return;
    int cap = h->chain_chunk > 0 ? std::min(h->chain_chunk, b.chain_cap) : b.chain_cap;
    if (call.chunks.cap > 0 && !h->deterministic) cap = std::min(cap, call.chunks.cap);
    const int s_ub = 60;   // squarings per interval at the most (a NaN iterate gets one)
    // 33..64 states: the whole chain in ONE launch, a workgroup per interval (dto_chain64.hip) -- no batched-GEMM launches, no
    // workspace chunks, the evaluation form chosen per interval on the device; the host reads back only what plans the sweep
    if (chain64_applies(h, b)) {
        ChainWork& w = b.chain;
        HIP_CHECK(hipMemsetAsync(w.smax, 0, 8 * sizeof(int32_t), st));
        HIP_CHECK(hipMemsetAsync(b.d_hump, 0, 8 * sizeof(unsigned long long), st));
        const int want_form = h->expm_form == 2 || h->expm_form == 3 ? h->expm_form : 0;
        {
            // priced at three powers + three more products per interval (either form, with its squarings, is 5..7 at these norms)
            ProfScope ps(h, st, CAT_CHAIN64, 6.0 * 2.0 * 64.0 * 64.0 * 64.0 * (double)nint);
            HIP_CHECK(launch_chain64(st, h->P, b.k, dZ, vals, w.norms, w.smax, w.d2max, w.s, s_ub, want_form, h->n_cu));
        }
        if (call.nothing_waits) {
            // the caller has planned and enqueued its sweep already: nothing on the host depends on this launch, the call stays
            // enqueue-only; the squaring count (a diagnostic) is read with the sweep statistics at the next entry point
            HIP_CHECK(hipMemcpyAsync(&h->mailbox->deferred_smax, w.smax, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            h->smax_pending = true;
            h->last_form = 0;
            if (call.in_bubble) call.in_bubble();
            if (call.chunks.done) call.chunks.done(0, (int)nint);
            if (call.after_last_enqueue) call.after_last_enqueue(0.0);
            return;
        }
        launch_hump(st, h->P, b.k, dZ, b.d_g1, h->P.kn_lo, (int)nint, w.norms, b.d_hump);
        const ChainReadback& rb = h->mailbox->chain;
        HIP_CHECK(hipMemcpyAsync(&h->mailbox->chain, w.smax, sizeof(ChainReadback), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(h->mailbox->hump, b.d_hump, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipEventRecord(h->ev_chain, st));
        if (call.in_bubble) call.in_bubble();
        HIP_CHECK(hipEventSynchronize(h->ev_chain));
        h->last_form = 0;   // per interval
        h->last_smax = rb.s_max2;
        read_hump(h, b);
        d2max = rb.d2max;
        if (call.chunks.done) call.chunks.done(0, (int)nint);
        if (call.after_last_enqueue) call.after_last_enqueue(d2max);
        return;
    }
    const double gemm_flops = 2.0 * npad * (double)npad * npad;
    h->last_smax = 0;
    // chunks of equal size (a multiple of 8 intervals) rather than full ones plus a remainder
    const int64_t nchunk = (nint + cap - 1) / cap;
    const int per = (int)std::min<int64_t>(cap, (((nint + nchunk - 1) / nchunk) + 7) / 8 * 8);
    for (int64_t c0 = 0; c0 < nint; c0 += per) {
        const int nb = (int)std::min<int64_t>(per, nint - c0);
        const int64_t int0 = h->P.kn_lo + c0;
        ChainWork& w = b.chain;
        const int nbpad = ((nb + 127) / 128) * 128;
        if (b.use_basis) {
            launch_fill(st, w.norms, (int64_t)nb * 4, INFINITY);  // ||A||_1 is not needed: alpha never exceeds d_2
            double* outs[3] = {w.W[1], w.W[2], w.W[3]};
            const size_t cs_set = (size_t)cap * npad * (npad / 64);  // every slot is written by the launch below: no clearing
            double* css[3] = {w.colsum, w.colsum + cs_set, w.colsum + 2 * cs_set};
            // (A_k as a fourth, degree-1 set of the launch below instead of k_build_A's streaming pass: measured slower,
            // 1.15 against 0.79 + 0.22 ms -- 8000 more tiles with one K panel each)
            {
                ProfScope ps(h, st, CAT_BUILD_A, 8.0 * npad * (double)npad * nb);   // one matrix written per interval
                launch_build_A(st, h->P, b.k, dZ, int0, nb, w.W[0]);
            }
            launch_basis_coef_multi(st, h->P, b.k, 3, b.basis, dZ, int0, nb, nbpad);
            {
                // A^2, A^3, A^4 in one launch (tiles interleaved: the write-bound sets overlap the MFMA-bound one)
                const double cols = b.basis[0].cntpad + b.basis[1].cntpad + b.basis[2].cntpad;
                ProfScope ps(h, st, CAT_BASIS_MULTI, 2.0 * npad * (double)npad * cols * nb);
                launch_basis_gemm_multi(st, npad, nb, nbpad, 3, b.basis, outs, css);
            }
            launch_norm_from_colsum_multi(st, npad, nb, 3, css, w.norms);
        } else {
            {
                ProfScope ps(h, st, CAT_BUILD_A, 8.0 * npad * (double)npad * nb);
                launch_build_A(st, h->P, b.k, dZ, int0, nb, w.W[0]);
            }
            { ProfScope ps(h, st, CAT_BGEMM, gemm_flops * nb); launch_bgemm_plain(st, npad, nb, w.W[0], w.W[0], w.W[1]); }
            { ProfScope ps(h, st, CAT_BGEMM, gemm_flops * nb); launch_bgemm_plain(st, npad, nb, w.W[0], w.W[1], w.W[2]); }
            { ProfScope ps(h, st, CAT_BGEMM, gemm_flops * nb); launch_bgemm_plain(st, npad, nb, w.W[1], w.W[1], w.W[3]); }
            launch_norm1(st, npad, nb, w);
        }
        HIP_CHECK(hipMemsetAsync(w.smax, 0, 8 * sizeof(int32_t), st));
        launch_expm_params(st, nb, s_ub, w);
        if (c0 == 0) HIP_CHECK(hipMemsetAsync(b.d_hump, 0, 8 * sizeof(unsigned long long), st));
        launch_hump(st, h->P, b.k, dZ, b.d_g1, int0, nb, w.norms, b.d_hump);
        // The evaluation form is decided ON THE DEVICE (k_expm_coef: three products + s3 squarings against two products + s
        // squarings, summed over the chunk) unless an option pins it, so the factor K of the first product can be
        // enqueued before the host knows the outcome; the host needs it only for the launch sequence that follows and reads
        // it back (with the squaring counts, 32 bytes) while the GPU works on K -- `in_bubble` adds more independent work.
        launch_expm_coef(st, nb, w, h->expm_form == 2 || h->expm_form == 3 ? h->expm_form : 0);
        // ... and it leaves on a stream of its own right behind k_expm_coef, so the host learns the form while the GPU is still
        // busy with K's GEMM (0.65 ms at 256 x 2000) and has the products enqueued before that GEMM ends: no bubble
        const ChainReadback& rb = h->mailbox->chain;
        HIP_CHECK(hipEventRecord(h->ev_rb, st));
        HIP_CHECK(hipStreamWaitEvent(h->stream_rb, h->ev_rb, 0));
        HIP_CHECK(hipMemcpyAsync(&h->mailbox->chain, w.smax, sizeof(ChainReadback), hipMemcpyDeviceToHost, h->stream_rb));
        HIP_CHECK(hipMemcpyAsync(h->mailbox->hump, b.d_hump, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream_rb));
        HIP_CHECK(hipEventRecord(h->ev_chain, h->stream_rb));
        if (b.use_basis) {
            launch_basis_coef(st, h->P, b.k, b.basis_all, dZ, int0, nb, nbpad, w.coef);
            ProfScope ps(h, st, CAT_OTHER, 2.0 * npad * (double)npad * b.basis_all.cntpad * nb);
            launch_basis_gemm(st, npad, nb, nbpad, b.basis_all, w.W[5], nullptr);
        } else {
            launch_poly_h3(st, npad, nb, w);
        }
        if (c0 == 0 && call.in_bubble) call.in_bubble();
        HIP_CHECK(hipEventSynchronize(h->ev_chain));
        const int form = rb.form;
        if (form != 2 && form != 3) throw HipError{"propagator chain: the evaluation form did not come back from the device"};
        h->last_form = form;
        // Y = A^4 K -> (Y + Pa, Y + Pb) in one launch
        { ProfScope ps(h, st, CAT_BGEMM_HORNER, gemm_flops * nb); launch_bgemm_poly(st, npad, nb, w, 3, 5, 4, COEF_PA, 6, COEF_PB); }
        const SlabDest slab{h->P, b.k, int0, vals};  // intervals with s_k = 0: the last product is exp(A_k) itself
        if (form == 2) {
            // T_16 = (Y + Pa)(Y + Pb) + Pc
            ProfScope ps(h, st, CAT_BGEMM_HORNER, gemm_flops * nb);
            launch_bgemm_poly(st, npad, nb, w, 4, 6, 5, COEF_PC, -1, 0, false, &slab);
        } else {
            // (L, R) = Ya Yb + weights of Ya + polynomials, then r = L R + Pe
            { ProfScope ps(h, st, CAT_BGEMM_HORNER, gemm_flops * nb); launch_bgemm_poly(st, npad, nb, w, 4, 6, 7, COEF_L, 8, COEF_R, true); }
            { ProfScope ps(h, st, CAT_BGEMM_HORNER, gemm_flops * nb); launch_bgemm_poly(st, npad, nb, w, 7, 8, 5, COEF_PC, -1, 0, false, &slab); }
        }
        const int s_max = form == 3 ? rb.s_max3 : rb.s_max2;
        const int s_sum = form == 3 ? rb.s_sum3 : rb.s_sum2;
        read_hump(h, b);  // accumulated over the chunks so far; final after the last one
        const double dv = rb.d2max;
        d2max = (dv == dv) ? std::max(d2max, dv) : dv;
        const double sq_flops = s_max > 0 ? gemm_flops * (double)s_sum / s_max : 0.0;
        h->last_smax = std::max(h->last_smax, s_max);
        int src = 5;
        for (int it = 0; it < s_max; ++it) {
            ProfScope ps(h, st, CAT_BGEMM_SQUARE, sq_flops);
            launch_bgemm_square(st, npad, nb, w, src, src == 4 ? 5 : 4, it, h->P, b.k, int0, vals);
            src = src == 4 ? 5 : 4;
        }
        if (call.chunks.done) call.chunks.done(c0, nb);  // the -E_k of these intervals are final behind what is enqueued now
    }
    if (call.after_last_enqueue) call.after_last_enqueue(d2max);
}

// max_k ||A_k^2||_1^(1/2), exact, for callbacks that do not run the propagator chain: A_k and A_k^2 only
// (one streaming pass + one small GEMM per chunk).  Sharper than the generator-norm bound, so the sweep
// usually needs a single round (q = 1).
// `higher`: also ||A^3||, ||A^4|| (store-less basis GEMMs) and return max_k min(d2, max(d3, d4)) -- the sharper growth
// rate of Al-Mohy & Higham's alpha_3, worth its cost only when d2 alone would force sub-stepping
double exact_d2(dto_handle* h, BilHost& b, const double* dZ, hipStream_t st, bool higher = false) {
    const int npad = b.k.npad;
    const int64_t nint = h->P.n_int;
    double d2max = 0.0;
    for (int64_t c0 = 0; c0 < nint; c0 += b.chain_cap) {
        const int nb = (int)std::min<int64_t>(b.chain_cap, nint - c0);
        const int64_t int0 = h->P.kn_lo + c0;
        ChainWork& w = b.chain;
        HIP_CHECK(hipMemsetAsync(w.smax, 0, 8 * sizeof(int32_t), st));
        launch_fill(st, w.norms, (int64_t)nb * 4, INFINITY);  // norms not computed below stay "unknown" for k_hump
        if (c0 == 0) HIP_CHECK(hipMemsetAsync(b.d_hump, 0, 8 * sizeof(unsigned long long), st));
        if (b.use_basis) {
            // ||A_k^2||_1 straight from the generator-subspace GEMM's fused column sums: neither A nor A^2 is
            // written (K = number of degree-2 products: a few GFLOP for all intervals)
            const int nbpad = ((nb + 127) / 128) * 128;
            const int nr = higher ? 3 : 1;
            for (int r = 0; r < nr; ++r) {
                double* cs = w.colsum + (size_t)r * b.chain_cap * npad * (npad / 64);
                launch_basis_coef(st, h->P, b.k, b.basis[r], dZ, int0, nb, nbpad, nullptr);
                launch_basis_gemm(st, npad, nb, nbpad, b.basis[r], nullptr, cs);
                launch_norm_from_colsum(st, npad, nb, cs, w.norms, 1 + r, higher ? nullptr : w.d2max);
            }
            if (higher) launch_beta_from_norms(st, nb, w);
        } else {
            launch_build_A(st, h->P, b.k, dZ, int0, nb, w.W[0]);
            launch_bgemm_plain(st, npad, nb, w.W[0], w.W[0], w.W[1]);
            launch_norm1_one(st, npad, nb, w, 1);
        }
        launch_hump(st, h->P, b.k, dZ, b.d_g1, int0, nb, w.norms, b.d_hump);
        // (the first 16 bytes of the readback: the two-product counts, which nothing reads here, and d2max)
        HIP_CHECK(hipMemcpyAsync(&h->mailbox->chain, w.smax, offsetof(ChainReadback, s_max3), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(h->mailbox->hump, b.d_hump, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const double dv = h->mailbox->chain.d2max;
        d2max = (dv == dv) ? std::max(d2max, dv) : dv;
    }
    read_hump(h, b);
    return d2max;
}

// Plan from the a-priori hump bound of k_hump: the fewest rounds whose Taylor sums cannot lose more than theta_v
// e-folds to cancellation; falls back to the growth-rate rule when no q <= 4 qualifies or the bound is not finite.
void read_hump(dto_handle* h, BilHost& b) {
    const unsigned long long* hp = h->mailbox->hump;
    b.hump_valid = true;
    for (int q = 0; q < 4; ++q) {
        double v;
        memcpy(&v, &hp[q], sizeof(double));
        b.hump_logH[q] = v;
        b.hump_kend[q] = (int)hp[4 + q];
        if (!(v == v)) b.hump_valid = false;
    }
}
SweepPlan plan_hump(const BilHost& b, double beta_fallback) {
    return dto::plan_hump(b.hump_valid, b.hump_logH, b.hump_kend, sweep_theta_v(), beta_fallback);
}

SweepPlan plan_from(dto_handle* h, BilHost& b, const double* dZ, hipStream_t st, bool loose = false) {
    Bounds bd = get_bounds(h, b, dZ, st);
    SweepPlan cheap;
    if (cheap_plan(bd, loose, cheap)) return cheap;
    // A cheap bound far beyond one round's radius (2.5 theta_v: a function of Z alone): ||A^2|| by itself will not settle q = 1 either,
    // so the pass over A^2 alone is skipped and the norms of A^2, A^3, A^4 are taken at once (1024 x 500, beta = 28.8: the A^2-only
    // pass was 1.4 of the 6.4 ms the exact norms cost a Hessian or an eval_constraint there)
    const bool straight = b.use_basis && bd.beta == bd.beta && bd.beta > 22.5;
    double d2 = exact_d2(h, b, dZ, st, straight);
    auto plan = [&] { return plan_hump(b, growth_rate(bd.beta, d2)); };
    if (!straight && d2 == d2 && plan().q > 1 && b.use_basis) d2 = exact_d2(h, b, dZ, st, true);  // ||A^3||, ||A^4|| sharpen the bound
    return plan();
}

// ------------------------------------------------------------------------------------------
// callbacks (device-pointer forms)
// ------------------------------------------------------------------------------------------

// Is every vector `now` bit-identical to its `cached` copy (both on the device)?  One round trip: the flag (a mailbox member) goes
// up as 1, one compare launch per pair clears it on a difference, it comes back, the host waits for it.
struct BitsPair { const double *now, *cached; int64_t n; };
bool bits_equal(hipStream_t st, std::initializer_list<BitsPair> pairs, int32_t* d_flag, int32_t* flag) {
    *flag = 1;
    HIP_CHECK(hipMemcpyAsync(d_flag, flag, sizeof(int32_t), hipMemcpyHostToDevice, st));
    for (const BitsPair& p : pairs) launch_bits_equal(st, p.now, p.cached, p.n, d_flag);
    HIP_CHECK(hipMemcpyAsync(flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return *flag != 0;
}

// The device half of a kept point (dto_kept_point.h; DevicePoint in dto_handle.h).  Its copies and its flag, once.
void alloc_point(dto_handle* h, DevicePoint& P, bool with_mu) {
    if (P.d_flag) return;
    P.d_Z = own(h, dalloc<double>((size_t)h->n_vars));
    if (with_mu) P.d_mu = own(h, dalloc<double>((size_t)std::max<int64_t>(h->n_cons, 1)));
    P.d_flag = own(h, dalloc<int32_t>(1));
}
// Is (dZ [, sigma] [, dmu] [, tag]) the point P keeps?  The host-side key first; then Z, and mu where the point holds one and one is
// given, bit for bit against the copies: one round trip.  On a miss the rebuild has BEGUN -- nothing is kept until keep_point.
bool at_kept_point(dto_handle* h, DevicePoint& P, hipStream_t st, const double* dZ, double sigma = 0.0, const double* dmu = nullptr, int32_t tag = 0) {
    bool hit = P.rec.may_hit(h->gen, tag, sigma, dmu == nullptr);
    if (hit && P.d_mu && dmu) hit = bits_equal(st, {{dZ, P.d_Z, h->n_vars}, {dmu, P.d_mu, h->n_cons}}, P.d_flag, &(h->mailbox->*P.flag));
    else if (hit) hit = bits_equal(st, {{dZ, P.d_Z, h->n_vars}}, P.d_flag, &(h->mailbox->*P.flag));
    if (!hit) P.rec.begin_rebuild();
    return hit;
}
// Closes the rebuild a miss began: the copies of Z and mu behind the rebuild's kernels, then the record.
void keep_point(dto_handle* h, DevicePoint& P, hipStream_t st, const double* dZ, double sigma = 0.0, const double* dmu = nullptr, int32_t tag = 0) {
    HIP_CHECK(hipMemcpyAsync(P.d_Z, dZ, sizeof(double) * (size_t)h->n_vars, hipMemcpyDeviceToDevice, st));
    if (P.d_mu && dmu && h->n_cons > 0) HIP_CHECK(hipMemcpyAsync(P.d_mu, dmu, sizeof(double) * (size_t)h->n_cons, hipMemcpyDeviceToDevice, st));
    P.rec.keep(h->gen, tag, sigma, dmu == nullptr);
}

void invalidate_sweep_caches(dto_handle* h) {
    for (auto& b : h->bil) b.cache.invalidate();
}

// reuse_forward_sweep: is dZ bit-identical to the point the cached sweeps were computed at?  If not, dZ becomes the new
// cache point and every integrator's cache is dropped.  (Not a KeptPoint of dto_kept_point.h and not to be folded into one: no
// generation, the new Z is adopted BEFORE the compute, and validity lives in SweepCache.)
bool same_point(dto_handle* h, const double* dZ, hipStream_t st) {
    if (!h->reuse) return false;
    if (!h->d_Zcache) {
        h->d_Zcache = own(h, dalloc<double>((size_t)h->n_vars));
        h->d_eq = own(h, dalloc<int32_t>(1));
    } else if (bits_equal(st, {{dZ, h->d_Zcache, h->n_vars}}, h->d_eq, &h->mailbox->same_flag)) {
        return true;
    }
    HIP_CHECK(hipMemcpyAsync(h->d_Zcache, dZ, sizeof(double) * (size_t)h->n_vars, hipMemcpyDeviceToDevice, st));
    invalidate_sweep_caches(h);
    return false;
}

// copy one of the caller's arrays of an external term (dto_set_external) into its device staging buffer
const double* ext_upload(dto_handle* h, int slot, int which, hipStream_t st) {
    ExtSlot& e = h->ext[slot];
    const double* src = which == 0 ? e.v.values : which == 1 ? e.v.first : e.v.second;
    static const char* what[3] = {"values", "first-derivative blocks", "second-derivative blocks"};
    if (!src)
        throw HipError{"external term " + std::to_string(slot) + ": " + what[which] +
                       " were not supplied (dto_set_external) -- the engine has no host fallback for closures"};
    if (!e.d[which]) e.d[which] = own(h, dalloc<double>(e.len[which]));
    HIP_CHECK(hipMemcpyAsync(e.d[which], src, e.len[which] * sizeof(double), hipMemcpyHostToDevice, st));
    return e.d[which];
}

// workgroups of a persistent-grid launch of `t` (k_tdb_mfma, k_tdb_kron and their product forms): its `resident`, lowered by
// option "tdb_resident" -- the scratch holds `resident` slots, a smaller grid uses the first ones
int tdb_grid(const dto_handle* h, const TdbHost& t) {
    return h->tdb_resident > 0 ? std::min(h->tdb_resident, t.resident) : t.resident;
}

// members per launch of an active time-dependent group: its cap from create, lowered by option "tdb_share_members"
int tdb_share_cap(const dto_handle* h, const TdbHost& t) {
    return h->tdb_share_members > 0 ? std::min(h->tdb_share_members, t.share_cap) : t.share_cap;
}

// Calls `f(first, count)` for the consecutive launches of an active group led by `lead`: `count` members from position `first` of
// lead.share_members, at most the cap each.
template <class F>
void tdb_share_launches(const dto_handle* h, const TdbHost& lead, F&& f) {
    const int cap = tdb_share_cap(h, lead), size = (int)lead.share_members.size();
    for (int first = 0; first < size; first += cap) f(first, std::min(cap, size - first));
}

// One launch of k_tdb_mfma for `count` integrators of one system (indices into h->tdb), intervals lo .. hi - 1.  A launch of one
// runs on that integrator's own description and scratch, a larger one on the leader's and the slots of the group launches.
void tdb_mfma_eval(dto_handle* h, const TdbHost& lead, const int* members, int count, const double* dZ, const double* dmu, int need,
                   int64_t lo, int64_t hi, hipStream_t st) {
    const TdbHost& t = count == 1 ? h->tdb[members[0]] : lead;
    KTdbGroup g{};
    g.count = count;
    for (int i = 0; i < count; ++i) {
        const TdbHost& mb = h->tdb[members[i]];
        g.m[i] = KTdbMember{mb.k.x_off, mb.k.row_off, mb.d_vals, mb.d_jac, mb.d_hess};
    }
    ProfScope ps(h, st, CAT_TDB_MFMA, tdb_mfma_flops(t.k, need, count) * (double)std::max<int64_t>(hi - lo, 0));
    HIP_CHECK(launch_tdb_mfma(st, h->P, t.k, g, t.d_Bp, t.d_BpT, dZ, dmu, need, lo, hi - lo, count == 1 ? t.d_scratch : t.d_share_scratch,
                              count == 1 ? t.stride : t.share_stride, tdb_grid(h, t)));
}

// blocks of a device-evaluated time-dependent bilinear integrator: the owned intervals for the defect; for the Jacobian /
// Hessian also the interval left of the first owned knot, whose z_{k+1} half lands in that knot's columns.  An active group
// (DTO_FLAG_SHARED_GENERATORS) is evaluated at its leader's turn -- the first member in list order, which every caller
// reaches first -- by launches that write the blocks of all members; a follower's turn finds its blocks written.
void tdb_eval(dto_handle* h, TdbHost& t, const double* dZ, const double* dmu, int need, hipStream_t st) {
    const KProb& P = h->P;
    const int64_t lo = need == 0 ? P.kn_lo : std::max<int64_t>(0, P.kn_lo - 1);
    const int64_t hi = need == 0 ? P.kn_lo + P.n_int : std::min<int64_t>(P.K, P.kn_lo + P.n_knots);
    if (t.kron) {
        ProfScope ps(h, st, CAT_TDB_KRON, tdb_kron_flops(t.k, t.kk, need) * (double)std::max<int64_t>(hi - lo, 0));
        HIP_CHECK(launch_tdb_kron(st, P, t.k, t.kk, dZ, dmu, need, lo, hi - lo, t.d_vals, t.d_jac, t.d_hess, t.d_scratch, t.stride, tdb_grid(h, t)));
    } else if (!t.mfma) {
        HIP_CHECK(launch_tdb(st, P, t.k, dZ, dmu, need, lo, hi - lo, t.d_vals, t.d_jac, t.d_hess, t.d_scratch, t.stride));
    } else if (!t.share_active || tdb_share_cap(h, t) < 2) {
        const int self = (int)(&t - h->tdb.data());
        tdb_mfma_eval(h, t, &self, 1, dZ, dmu, need, lo, hi, st);
    } else if (t.share_leader == (int)(&t - h->tdb.data())) {
        tdb_share_launches(h, t, [&](int first, int count) {
            tdb_mfma_eval(h, t, t.share_members.data() + first, count, dZ, dmu, need, lo, hi, st);
        });
    }
}

// Matrix-free products of a device time-dependent integrator, dense or structured (option "tdb_matrix_free_products"): its rows of
// J w, or its part of J' w added into the zero-filled dy -- staged per interval, then placed by one thread per entry.  No block, no
// slab.  One record under "tdb_product" whichever kernel runs (the structured one does not count under "tdb_kron").
void tdb_product(dto_handle* h, TdbHost& t, const double* dZ, const double* dw, double* dy, int transpose, hipStream_t st) {
    const KProb& P = h->P;
    const int need = transpose ? 4 : 3;
    const double flops = t.kron ? tdb_kron_flops(t.k, t.kk, need) : (t.mfma ? tdb_mfma_flops(t.k, need) : tdb_product_flops(t.k, need));
    ProfScope ps(h, st, CAT_TDB_PRODUCT, flops * (double)std::max<int64_t>(P.K, 0));
    double* out = transpose ? t.d_jtv : dy;
    if (t.kron) HIP_CHECK(launch_tdb_kron_product(st, P, t.k, t.kk, dZ, dw, need, out, t.d_scratch, t.stride, tdb_grid(h, t)));
    else if (t.mfma) HIP_CHECK(launch_tdb_mfma_product(st, P, t.k, t.d_Bp, t.d_BpT, dZ, dw, need, out, t.d_scratch, t.stride, tdb_grid(h, t)));
    else HIP_CHECK(launch_tdb_product(st, P, t.k, dZ, dw, need, out, t.d_scratch, t.stride));
    if (transpose) HIP_CHECK(launch_tdb_jtv_place(st, P, t.k, dw, t.d_jtv, dy));
}

// One launch per layer of an objective term's listings (a single layer unless its `times` repeats a knot): within a launch no
// two listings touch the same gradient / Hessian entry, across launches the stream orders them -- fixed order of addition.
template <class F>
void for_layers(dto_handle* h, size_t i, F&& f, bool first_only = false) {
    const KObj& o = h->obj[i];
    const std::vector<int64_t>& ls = h->obj_info[i].layer_start;
    for (size_t l = 0; l + 1 < ls.size() && !(first_only && l > 0); ++l) {
        KObj ol = o;
        const int64_t i0 = ls[l];
        ol.n_times = ls[l + 1] - i0;
        ol.times += i0;
        if (ol.Qs) ol.Qs += i0;
        if (ol.last) ol.last += i0;
        if (ol.params) ol.params += i0 * ol.n_comps;
        f(ol);
    }
}

// structured bilinear integrator (dto_kron.hip): need 0 defect, 1 Jacobian block, 2 Hessian block of the owned intervals
void kron_eval(dto_handle* h, BilHost& b, const double* dZ, const double* dmu, int need, double* dg, double* dvals, double* dH, hipStream_t st) {
    HIP_CHECK(hipMemsetAsync(b.kk.stats, 0, 2 * sizeof(int32_t), st));
    const int cp = (b.kk.rw + 15) / 16 * 16, m = b.k.m;
    const int cols = need == 0 ? cp : (need == 1 ? (1 + m) * cp + b.kk.bp : (2 + 2 * m + m * (m + 1) / 2) * cp);
    // priced at sixteen terms of 2 bp^2 per column and (on average two) sources
    ProfScope ps(h, st, need == 2 ? CAT_SWEEP_ADJOINT : CAT_SWEEP, 2.0 * b.kk.bp * b.kk.bp * cols * 2.0 * 16.0 * (double)h->P.n_int);
    HIP_CHECK(launch_kron(st, h->P, b.k, b.kk, dZ, dmu, need, dg, dvals, dH, b.d_kron_scratch, b.kron_stride));
}

// ... and its product modes: the integrator's rows of J w (transpose = 0) or its part of J' w into the zero-filled dy; no value slab
void kron_product(dto_handle* h, BilHost& b, const double* dZ, const double* dw, double* dy, int transpose, hipStream_t st) {
    HIP_CHECK(hipMemsetAsync(b.kk.stats, 0, 2 * sizeof(int32_t), st));
    const int cp = (b.kk.rw + 15) / 16 * 16;
    ProfScope ps(h, st, CAT_JAC_PRODUCT, 2.0 * b.kk.bp * b.kk.bp * ((b.k.m + 2) * cp) * 2.0 * 16.0 * (double)h->P.n_int);
    HIP_CHECK(launch_kron(st, h->P, b.k, b.kk, dZ, dw, transpose ? 4 : 3, dy, nullptr, nullptr, b.d_kron_scratch, b.kron_stride));
}
// the same two products on the small path (dto_small.hip): exp(A) w_x as one more forward column, exp(A)' w_k as an adjoint column
void small_product(dto_handle* h, BilHost& b, const double* dZ, const double* dw, double* dy, int transpose, hipStream_t st) {
    SweepTypes ty = make_types(b.k.m, false);
    if (!transpose) ty.t[ty.T++] = TypeDesc{0, {0, 0}, {0, 0}, {0, 0}};
    ProfScope ps(h, st, CAT_JAC_PRODUCT, 2.0 * b.k.n * b.k.n * (b.k.m + 2) * 2.0 * 16.0 * (double)h->P.n_int);
    HIP_CHECK(launch_small(st, h->P, b.k, b.d_Gs, ty, make_types(0, false), dZ, dw, dy, nullptr, nullptr, transpose ? 16 : 8));
}

void do_objective(dto_handle* h, const double* dZ, double* df, hipStream_t st) {
    HIP_CHECK(hipMemsetAsync(df, 0, sizeof(double), st));
    for (auto& o : h->obj) launch_objective(st, h->P, o, dZ, h->d_partial, df);
    for (auto& e : h->ext_obj)
        if (e.k.n_list > 0) launch_ext_objective(st, e.k, e.weight, ext_upload(h, e.ext_slot, 0, st), df);
}

void do_gradient(dto_handle* h, const double* dZ, double* dgrad, hipStream_t st) {
    HIP_CHECK(hipMemsetAsync(dgrad, 0, sizeof(double) * (size_t)h->info.grad_len, st));
    for (size_t i = 0; i < h->obj.size(); ++i)
        for_layers(h, i, [&](const KObj& ol) { launch_gradient(st, h->P, ol, dZ, dgrad); });
    for (auto& e : h->ext_obj)
        if (e.k.n_list > 0) launch_ext_gradient(st, h->P, e.k, e.weight, ext_upload(h, e.ext_slot, 1, st), dgrad);
}

// after a stored sweep of the p column alone: its terms stay valid for later callbacks at the same point, so their counts per block
// move out of the way of the next sweep (b.cache's recorder of that sweep does the bookkeeping)
void keep_p_column_counts(BilHost& b, hipStream_t st) {
    HIP_CHECK(hipMemcpyAsync(b.fw.nterms_p, b.fw.nterms, sizeof(int32_t) * b.fw.Kpad, hipMemcpyDeviceToDevice, st));
}

void do_constraint(dto_handle* h, const double* dZ, double* dg, hipStream_t st) {
    const bool same = same_point(h, dZ, st);
    for (auto& b : h->bil) {
        if (b.kron) { kron_eval(h, b, dZ, nullptr, 0, dg, nullptr, nullptr, st); continue; }
        if (b.small) {
            HIP_CHECK(launch_small(st, h->P, b.k, b.d_Gs, make_types(0, false), make_types(0, false), dZ, nullptr, dg, nullptr, nullptr, 1));
            continue;
        }
        if (h->P.n_int > 0) {
            SweepChoice alone;
            const bool have_sums = b.cache.at(same).has_p_sums();
            if (!have_sums && s64_plans_itself(h, b, b.fw, make_types(0, false), &alone)) {
                // 33..64 states: the one-launch sweep takes its step budget from the norm bound ON THE DEVICE (k_plan_dev: the
                // formulas of cheap_plan / plan_sweep) -- the call no longer waits 40 us for eight bytes
                enqueue_bounds(h, b, dZ, st);
                launch_plan_dev(st, reinterpret_cast<const unsigned long long*>(h->d_bounds), h->d_plan);
                run_sweep(h, b, b.fw, make_types(0, false), dZ, nullptr, PLAN_ON_DEVICE, st, SweepArgs().as_chosen(alone).planned_on_device(h->d_plan));
                b.cache.constraint_swept_on_device_plan(b.fw.nblk);
            } else if (!have_sums) {  // else exp(A)x of this very point is still in b.fw.S
                SweepPlan plan = plan_from(h, b, dZ, st, /*loose=*/true);
                if (plan.tc >= 0 && h->reuse && b.pairing && plan.d_ub + 1 > b.fw.dcap) plan = plan_from(h, b, dZ, st);  // the term store is what limits
                SweepTypes ty = make_types(0, false);
                // with reuse on, the terms of the p column are kept: a Jacobian at this point then sweeps its tangent
                // columns alone and a Hessian needs no forward sweep at all
                const bool keep_p = h->reuse && b.pairing && plan.q == 1 && plan.d_ub + 1 <= b.fw.dcap;
                const int steps = run_sweep(h, b, b.fw, ty, dZ, nullptr, plan, st, SweepArgs().keep_terms(keep_p));
                b.cache.constraint_swept(h->reuse, keep_p, steps, b.fw.nblk);
                if (keep_p) keep_p_column_counts(b, st);
            }
            launch_cons_bilinear(st, h->P, b.k, b.fw, dZ, dg);
        }
    }
    for (auto& d : h->der) launch_cons_derivative(st, h->P, d, dZ, dg);
    for (size_t i = 0; i < h->ext_int.size(); ++i)
        if (h->P.n_int > 0) launch_extint_cons(st, h->P, h->ext_int[i], ext_upload(h, (int)i, 0, st), dg);
    for (auto& t : h->tdb)
        if (h->P.n_int > 0) { tdb_eval(h, t, dZ, nullptr, 0, st); launch_extint_cons(st, h->P, t.place, t.d_vals, dg); }
    for (auto& c : h->con) {
        if (!c.external) launch_cons_knot(st, h->P, c.k, dZ, dg);
        else if (c.k.n_times > 0) launch_ext_cons(st, c.k, ext_upload(h, c.ext_slot, 0, st), dg);
    }
}

// DTO_FLAG_SHARED_GENERATORS: -E_k of intervals int0 .. int0 + nb - 1, final in the leader's positions behind what `st` holds, to
// the positions of the group's other members
void share_blocks(dto_handle* h, BilHost* const* members, int n_members, int64_t int0, int nb, double* dvals, hipStream_t st) {
    KShare sh{};
    sh.n = members[0]->k.n;
    sh.nf = n_members - 1;
    for (int i = 0; i < n_members; ++i) { sh.x_off[i] = members[i]->k.x_off; sh.pre[i] = members[i]->k.pre; }
    // priced by the bytes it writes: one block per follower and interval (it reads one more block per interval)
    ProfScope ps(h, st, CAT_SHARE, 8.0 * sh.n * (double)sh.n * nb * sh.nf);
    launch_share_E(st, h->P, sh, int0, nb, dvals);
}

// A single bilinear integrator, on the general path, with intervals to own: the propagator chain alone writes its -E_k blocks, so
// do_jacobian clears around them and build_jac_plan hands each block over with its chain chunk -- one predicate for both
bool lone_general_bilinear(const dto_handle* h) {
    return h->bil.size() == 1 && h->P.n_int > 0 && !h->bil[0].small && !h->bil[0].kron;
}

// `caller`: a cap on the chain's chunks and a callback per finished chunk, for every chain this call runs (the host-pointer
// Jacobian ships a lone integrator's blocks early with them)
void do_jacobian(dto_handle* h, const double* dZ, double* dvals, hipStream_t st, const ChainChunks& caller = {}) {
    // fill!(∂, 0), evaluator.jl:497 -- the -E_k block of a lone bilinear integrator is skipped: the chain
    // overwrites all of it
    // (enqueued inside the chain, where it fills the GPU while the host waits for the scaling decision)
    const bool lone = lone_general_bilinear(h);
    // bound and primed output (dto_bind_output_dev): constants are in place, clear only the runs kernels accumulate into
    const bool keep_constants = h->bound[0] == dvals && h->primed[0] && ensure_bind_runs(h, 0);
    if (keep_constants) launch_zero_runs(st, h->d_bind_start[0], h->d_bind_len[0], h->n_bind_runs[0], dvals);
    else if (!lone) {
        ProfScope ps(h, st, CAT_ZERO, 8.0 * (double)h->info.jac_len);
        HIP_CHECK(hipMemsetAsync(dvals, 0, sizeof(double) * (size_t)h->info.jac_len, st));
    }
    h->last_terms = 0;
    const bool same = same_point(h, dZ, st);
    for (auto& b : h->bil) {
        if (b.kron) { kron_eval(h, b, dZ, nullptr, 1, nullptr, dvals, nullptr, st); continue; }
        if (b.small) {
            HIP_CHECK(launch_small(st, h->P, b.k, b.d_Gs, make_types(b.k.m, false), make_types(0, false), dZ, nullptr, nullptr, dvals, nullptr, 2));
            continue;
        }
        Bounds bd{0, 0};
        // DTO_FLAG_SHARED_GENERATORS: the leader of an active group runs the one chain; its followers' sweeps are enqueued where
        // its own is -- planned from the leader's bounds and the leader's chain readback, which are functions of the generators, u
        // and dt alone -- and k_share_E copies every finished chunk of -E_k blocks to the followers' positions on the chain's
        // stream.  A follower has been swept and filled by the time the loop reaches it (the leader comes first in list order,
        // and the join below covers the whole group): it only writes its tangent columns.
        // (with the flag clear: the integrator alone, nothing allocated, no hook installed)
        BilHost* members[1 + SHARE_MAX_FOLLOWERS] = {&b};
        int n_members = 1;
        for (int f : b.share_followers) members[n_members++] = &h->bil[f];
        if (h->P.n_int > 0 && !b.follows()) {
            // generator-norm bounds: enqueued here, read inside the chain's own readback point (no stream sync of their
            // own); the squaring cap they used to provide is the constant 60, a NaN iterate gets one squaring
            enqueue_bounds(h, b, dZ, st);
            // The sweep (one persistent launch, no HBM traffic to speak of) runs on the second stream next to the polynomial
            // products and squarings of the chain: its 223 workgroups leave 33 CUs idle and every chain launch has a tail --
            // together 5-6 % of the call (12.3 -> 11.5 ms at 256 x 2000).  Option "overlap_sweep" = 0 runs one kernel at a
            // time (per-kernel timings mean something only then).
            // (from 512 states on the step-per-launch sweep's small launches only get in the way of the chain's big ones:
            // 18.7 -> 19.3 ms at 512 x 500, 71.1 -> 72.5 ms at 1024 x 300; below, 3-6 % faster: tools/overlap_by_size.py)
            const bool overlap = h->overlap_sweep != 0 && b.k.npad < 512;
            hipStream_t ss = overlap ? h->stream2 : st;
            if (overlap) {
                HIP_CHECK(hipEventRecord(h->ev_fork, st));  // dZ (and the zero-filled slab) are ready here
                HIP_CHECK(hipStreamWaitEvent(ss, h->ev_fork, 0));
            }
            auto sweep_one = [&](BilHost& mb, SweepPlan plan, const int32_t* plan_dev) {
                SweepTypes ty = make_types(mb.k.m, false);
                const auto held = mb.cache.at(same);
                // the p column of this very point is stored (eval_constraint or a Hessian came first)
                const bool have_p = held.has_p_column() && plan.q == 1;
                // ... but where the whole sweep runs as ONE persistent launch beside the chain, sweeping all columns again is
                // cheaper than the step-per-launch form the frozen variant needs (256 x 2000: 10.9 against 12.0 ms per Jacobian);
                // the stored p terms stay valid for a Hessian at this point either way (a sweep without store leaves them alone)
                // (asked for the sweep without store beside the chain: what sweep_fused_plan accepts for a sweep alone it accepts there too
                // -- it only tries the eight-wavefront search first, the 64-state instance changes its interval count, not its answer)
                const bool beside_chain = overlap && !h->deterministic;
                const bool one_launch = choose_sweep(h, mb, mb.fw, ty, plan, /*store=*/false, beside_chain).form != SWEEP_STEP;
                if (have_p && !one_launch) {
                    // sweep the tangent columns alone, their inhomogeneous terms read the stored p terms
                    SweepBuf wf = mb.fw;
                    wf.frozen = mb.fw.Zt;
                    wf.frozen_total = held.p_column_steps() + 1;
                    wf.first_type = 1;
                    run_sweep(h, mb, wf, ty, dZ, nullptr, plan, ss);
                    launch_apply_Gu(ss, mb.k, mb.fw, 0, mb.fw.S, mb.fw.GY);
                    mb.cache.jacobian_swept_frozen();
                    return;
                }
                // with reuse on and a Hessian to follow, keep every Taylor term so that the Hessian can skip its forward sweep
                // (not when the p terms are there already: they are all the Hessian's pairing takes from the forward sweep)
                const bool keep = h->reuse && mb.pairing && plan.q == 1 && plan.d_ub + 1 <= mb.fw.dcap && !have_p;
                // (option "deterministic": the sweep keeps the shape it has when it runs alone, so the bits do not depend on
                // overlap_sweep; next to the chain the 256-state sweep otherwise groups its intervals by twelve instead of nine)
                // (a short shard's sweep in the generator-stationary form wants the chip to itself for a fraction of a millisecond: it
                // follows the chain on the call's stream instead of sharing the chip with it)
                SweepChoice choice = choose_sweep(h, mb, mb.fw, ty, plan, keep, /*shared_chip=*/false);
                const bool gs_alone = choice.form == SWEEP_GS;
                hipStream_t sw = gs_alone ? st : ss;
                if (beside_chain && !gs_alone) choice = choose_sweep(h, mb, mb.fw, ty, plan, keep, /*shared_chip=*/true);
                const int steps = run_sweep(h, mb, mb.fw, ty, dZ, nullptr, plan, sw, SweepArgs().as_chosen(choice).planned_on_device(plan_dev));
                launch_apply_Gu(sw, mb.k, mb.fw, 0, mb.fw.S, mb.fw.GY);
                mb.cache.jacobian_swept(h->reuse, keep, plan.q, steps);  // (keep: the store now holds every column type; q > 1: the scale factors changed)
            };
            auto sweep_with = [&](SweepPlan plan, const int32_t* plan_dev = nullptr) {
                for (int i = 0; i < n_members; ++i) sweep_one(*members[i], plan, plan_dev);
            };
            // One-launch chain (33..64 states): the chain's exact norms arrive only when ALL of it is done, so a sweep planned from
            // them would run behind it.  Where the cheap bound already gives a single round, the sweep is planned from that bound
            // (as eval_constraint and the Hessian do) and enqueued FIRST, on the second stream: its workgroups and the chain's
            // share the CUs (64 x 1000: 0.42 -> 0.3x ms per Jacobian).
            bool swept = true;  // the tangent sums of this very point are still in b.fw (of every member; members[0] is always there)
            for (int i = 0; i < n_members; ++i) swept = swept && members[i]->cache.at(same).has_tangent_sums();
            // every entry but the -E_k blocks, which the chain overwrites: once per call, behind the early sweep on ITS stream or in
            // the chain's bubble on the call's
            bool zeroed = false;
            auto zero_around_blocks = [&](hipStream_t s) {
                if (!lone || keep_constants || zeroed) return;
                ProfScope ps(h, s, CAT_ZERO, 8.0 * ((double)h->info.jac_len - (double)h->P.n_int * b.k.n * b.k.n));
                launch_jac_zero(s, h->P, b.k, dvals);
                zeroed = true;
            };
            static const int early_on = tune_int("DTO_SWEEP_EARLY", 1);  // A/B runs (TUNING builds)
            if (!swept && early_on && chain64_applies(h, b) && s64_plans_itself(h, b, b.fw, make_types(b.k.m, false))) {
                // ... and planned on the device: the whole call is enqueue-only
                launch_plan_dev(st, reinterpret_cast<const unsigned long long*>(h->d_bounds), h->d_plan);
                HIP_CHECK(hipEventRecord(h->ev_fork, st));   // the plan is ready here
                if (overlap) HIP_CHECK(hipStreamWaitEvent(ss, h->ev_fork, 0));
                sweep_with(PLAN_ON_DEVICE, h->d_plan);
                swept = true;
                // the fill behind the sweep on ITS stream: only the tangent-column writers after the join need it, and the chain
                // (which skips nothing the fill touches) starts 28 us earlier than with the fill in front of it
                zero_around_blocks(ss);
            }
            if (!swept && early_on && chain64_applies(h, b)) {   // (with or without overlap: the plan, hence the bits, must not depend on it)
                HIP_CHECK(hipStreamSynchronize(st));
                bd = read_bounds(h);
                SweepPlan early;
                if (cheap_plan(bd, /*loose=*/true, early)) {
                    sweep_with(early);
                    swept = true;
                    zero_around_blocks(ss);  // (the fill no longer has a host wait to hide in: it goes behind the sweep, on the sweep's stream)
                }
            }
            const bool nothing_waits = swept && chain64_applies(h, b);
            ChainCall call;
            call.chunks = caller;
            // a group's copy follows each chunk of the chain; the caller's own callback comes after it
            if (n_members > 1)
                call.chunks.done = [&](int64_t c0, int nb) {
                    share_blocks(h, members, n_members, h->P.kn_lo + c0, nb, dvals, st);
                    if (caller.done) caller.done(c0, nb);
                };
            call.in_bubble = [&] { zero_around_blocks(st); };
            call.nothing_waits = nothing_waits;
            call.after_last_enqueue = [&](double d2) {
                bd = read_bounds(h);  // copied before the chain's readback event
                // ||A^t|| <= ||A^2||^floor(t/2) ||A||^(t mod 2): the exact d2 of the chain is the sharper
                // (and still rigorous) growth rate for the sweep's step budget
                if (swept) return;
                const SweepPlan from_chain = plan_hump(b, growth_rate(bd.beta, d2));
                if (h->reuse)   // a Hessian at this very point need not buy the norms again
                    for (int i = 0; i < n_members; ++i) members[i]->cache.chain_planned(from_chain.q, from_chain.d_ub);
                sweep_with(from_chain);
            };
            run_chain(h, b, dZ, dvals, st, call);
            if (overlap) {
                HIP_CHECK(hipEventRecord(h->ev_join, ss));
                HIP_CHECK(hipStreamWaitEvent(st, h->ev_join, 0));
            }
        }
        {
            // tangent columns (m + 1 per interval: u_j and dt) and the identity of the z_{k+1} half
            ProfScope ps(h, st, CAT_ASSEMBLY, 8.0 * (double)h->P.n_int * b.k.n * (b.k.m + 2 + b.k.m + 1));
            launch_jac_bilinear(st, h->P, b.k, b.fw, dvals);
        }
    }
    for (auto& d : h->der) launch_jac_derivative(st, h->P, d, dZ, dvals);
    for (size_t i = 0; i < h->ext_int.size(); ++i)
        launch_extint_jac(st, h->P, h->ext_int[i], ext_upload(h, (int)i, 1, st), dvals);
    for (auto& t : h->tdb) { tdb_eval(h, t, dZ, nullptr, 1, st); launch_extint_jac(st, h->P, t.place, t.d_jac, dvals); }
    for (auto& c : h->con) {
        if (!c.external) launch_jac_knot(st, h->P, c.k, dZ, dvals);
        else if (c.k.n_times > 0) launch_ext_jac(st, c.k, ext_upload(h, c.ext_slot, 1, st), dvals);
    }
}

void do_hessian(dto_handle* h, const double* dZ, double sigma, const double* dmu, double* dH, hipStream_t st) {
    static const int zero_beside_on = tune_int("DTO_HESS_ZERO_BESIDE", 1);  // A/B runs (TUNING builds)
    // (worth an event round only for a large slab: 5.57 -> 5.49 ms at 256 x 2000, +4 us at 64 x 1000 and 256 x 250)
    const bool zero_beside = zero_beside_on && h->overlap_sweep != 0 && h->P.n_int > 0 && !h->bil.empty() && !h->bil[0].small &&
                             (size_t)h->info.hess_len * sizeof(double) >= ((size_t)256 << 20) &&
                             !h->integ_kind.empty() && h->integ_kind[0] == DTO_INTEGRATOR_BILINEAR;
    bool zero_joined = true;
    // bound output, or the private slab of the Hessian-vector products: structural zeros are in place
    if (((h->bound[1] == dH && h->primed[1]) || (dH == h->hp_slab && h->hp_slab_primed)) && ensure_bind_runs(h, 1))
        launch_zero_runs(st, h->d_bind_start[1], h->d_bind_len[1], h->n_bind_runs[1], dH);
    else if (zero_beside) {
        // fill!(H, 0), evaluator.jl:571 -- on the second stream: the fill is HBM-bound, the sweeps that open the bilinear block
        // are MFMA-bound and write nothing into H, so the 1.7 GB (256 x 2000) are cleared underneath them; the first kernel
        // that writes H waits for it (need_zero)
        HIP_CHECK(hipEventRecord(h->ev_fork, st));  // whatever used H before on this stream is done
        HIP_CHECK(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
        {
            ProfScope ps(h, h->stream2, CAT_ZERO, 8.0 * (double)h->info.hess_len);
            HIP_CHECK(hipMemsetAsync(dH, 0, sizeof(double) * (size_t)h->info.hess_len, h->stream2));
        }
        HIP_CHECK(hipEventRecord(h->ev_zero, h->stream2));
        zero_joined = false;
    } else {
        ProfScope ps(h, st, CAT_ZERO, 8.0 * (double)h->info.hess_len);
        HIP_CHECK(hipMemsetAsync(dH, 0, sizeof(double) * (size_t)h->info.hess_len, st));  // fill!(H, 0), evaluator.jl:571
    }
    auto need_zero = [&] {
        if (!zero_joined) { HIP_CHECK(hipStreamWaitEvent(st, h->ev_zero, 0)); zero_joined = true; }
    };
    const bool same = same_point(h, dZ, st);
    // integrators in reference order (evaluator.jl:574-598)
    for (size_t i = 0; i < h->integ_kind.size(); ++i) {
        if (h->integ_kind[i] == DTO_INTEGRATOR_BILINEAR) {
            BilHost& b = h->bil[h->integ_index[i]];
            if (h->P.n_int <= 0) continue;
            if (b.kron) {
                need_zero();
                kron_eval(h, b, dZ, dmu, 2, nullptr, nullptr, dH, st);
                continue;
            }
            if (b.small) {
                need_zero();
                HIP_CHECK(launch_small(st, h->P, b.k, b.d_Gs, make_types(b.k.m, true), make_types(b.k.m, false), dZ, dmu, nullptr, nullptr, dH, 4));
                continue;
            }
            // (the budget from the cheap bound serves while the term store holds it: the sweeps end by their own test, and the
            // pairing loops run over the terms actually produced -- the exact norms cost a store-less basis GEMM and two round trips)
            // (reuse_forward_sweep, same point as the last Jacobian: the chain's exact norms have planned that call's sweep already --
            // at 1024 states the passes that establish q = 1 for a Hessian on its own are 4.9 of its 29.5 ms)
            const auto held = b.cache.at(same);
            SweepPlan plan = held.has_plan() ? SweepPlan{held.plan_rounds(), held.plan_budget()} : plan_from(h, b, dZ, st, /*loose=*/b.pairing);
            if (plan.tc >= 0 && plan.d_ub + 1 > b.fw.dcap) plan = plan_from(h, b, dZ, st);
            const bool pair = b.pairing && plan.q == 1 && plan.d_ub + 1 <= b.fw.dcap;
            const int m = b.k.m, T1 = 1 + m;
            int steps_f, Tf = T1, nblk_p = 0;  // Tf: types per stored forward term; nblk_p: intervals per entry of fw.nterms_p (Tf == 1)
            SweepTypes ty1 = make_types(m, false);
            // Pairing path with a forward sweep of its own: the adjoint sweep is one persistent launch that leaves CUs idle, the
            // forward sweep of the p column a host-driven sequence of small launches -- independent until the pairing kernels,
            // so the adjoint sweep is enqueued first and the forward sweep runs next to it on the second stream.
            const bool fwd_needed = pair && !(held.has_all_terms() || held.has_p_column());
            // (where the adjoint sweep has no single-workgroup form -- short shards -- both sweeps take the generator-stationary form,
            // one after the other; beside a fused adjoint sweep the forward column keeps its step launches, which fit into the CUs
            // that sweep leaves idle: measured 5.5 against 5.9 ms at 256 x 2000 with the forward column first and alone)
            // (option "deterministic": never side by side -- beside the adjoint sweep the forward column takes another form, step
            // launches instead of the generator-stationary sweep at 128 / 256 states, another interval grouping at 33..64, so its
            // summation order would follow overlap_sweep)
            // the adjoint sweep's form, chosen as for a sweep alone on the chip either way: the eight-wavefront shape it would take as
            // a neighbour, leaving more CUs to the forward sweep's launches, measured 5.9 against 5.7 ms
            const SweepChoice adjoint = choose_sweep(h, b, b.ad, ty1, plan, /*store=*/pair, /*shared_chip=*/false);
            SweepArgs aa = SweepArgs().adjoint(CAT_SWEEP_ADJOINT).as_chosen(adjoint);
            const bool side_by_side = fwd_needed && h->overlap_sweep && !h->deterministic && adjoint.one_workgroup();
            bool adjoint_enqueued = false;
            if (side_by_side) {
                HIP_CHECK(hipEventRecord(h->ev_fork, st));  // dZ, dmu and the zeroed slab are ready here
                HIP_CHECK(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
                run_sweep(h, b, b.ad, ty1, dZ, dmu, plan, st, aa);   // enqueue only: the steps it took are read below
                adjoint_enqueued = true;
            }
            hipStream_t sf = side_by_side ? h->stream2 : st;
            if (pair) {
                // Pairing path: every tangent comes from the ADJOINT sweep (the (x,u) block needs those anyway); of the forward
                // sweep only the Taylor terms of the p column are used (k_hess_pair, k_hess_bilinear).
                if (held.has_all_terms()) {
                    steps_f = held.all_terms_steps();  // the Jacobian of this very point stored every forward term
                } else if (held.has_p_column()) {
                    Tf = 1;
                    steps_f = held.p_column_steps();   // eval_constraint (or an earlier Hessian) stored the p terms of this point
                    nblk_p = held.p_column_nblk();     // (a frozen Jacobian sweep in between re-used fw.nterms and fw.nblk)
                } else {
                    Tf = 1;
                    steps_f = run_sweep(h, b, b.fw, make_types(0, false), dZ, nullptr, plan, sf, SweepArgs().keep_terms(true).beside_others(side_by_side));
                    nblk_p = b.fw.nblk;
                    b.cache.hessian_swept_p_column(h->reuse, steps_f, nblk_p);  // the p sums are valid, the tangent sums are not
                    keep_p_column_counts(b, sf);
                }
                launch_apply_generators(sf, b.k, b.fw, 0, b.fw.Zt, b.fw.W);  // V_l = G_l x (term 0 of the p column is x)
                if (side_by_side) {
                    HIP_CHECK(hipEventRecord(h->ev_join, sf));
                    HIP_CHECK(hipStreamWaitEvent(st, h->ev_join, 0));
                }
            } else {
                steps_f = run_sweep(h, b, b.fw, make_types(m, true), dZ, nullptr, plan, st);
                launch_apply_Gu(st, b.k, b.fw, 0, b.fw.S, b.fw.GY);
                b.cache.hessian_swept_second_order();  // this sweep re-initialised the scale factors for its own q
                // W_j = G_j' mu from the adjoint sweep's term-0 buffer
                launch_sweep_init(st, h->P, b.k, b.ad, make_types(0, false), dZ, dmu, 1, plan.q);
                launch_apply_generators(st, b.k, b.ad, 1, b.ad.Z[0], b.ad.W);
            }
            const int steps_a = adjoint_enqueued ? fused_sweep_steps(h, b.ad, plan.d_ub, st)
                                                 : run_sweep(h, b, b.ad, ty1, dZ, dmu, plan, st, aa.wait_for_steps(pair));
            if (h->profiling && pair)
                // the fused launch was priced by its step budget; now that the terms it ran are known, price it by those: 2 npad^2
                // (m+1) generator products per column and term, (1+m) column types (the flops bench.py's roofline uses)
                for (auto it = h->prof.rbegin(); it != h->prof.rend(); ++it)
                    if (it->cat == CAT_SWEEP_ADJOINT) {
                        if (it->flops > 0.0) it->flops = 2.0 * b.k.npad * (double)b.k.npad * b.ad.Kpad * (m + 1) * T1 * steps_a * plan.q;
                        break;
                    }
            launch_apply_Gu(st, b.k, b.ad, 1, b.ad.S, b.ad.GY);
            need_zero();
            launch_hess_bilinear(st, h->P, b.k, b.fw, b.ad, dmu, dH, pair ? 0 : 1);
            if (pair) {
                // (u_i,u_j) block from the stored Taylor terms (no second-order columns): Beta-weighted sums U_a of the
                // forward p terms, G_j U_a, then dot products with the adjoint tangent terms
                const int nf = steps_f + 1, na = steps_a + 1;
                const int64_t typesz = (int64_t)b.fw.Kpad * b.k.npad;
                const int64_t cols = (int64_t)na * b.fw.Kpad;  // one type of every stored term
                SweepBuf plain = b.fw;
                if (Tf == 1) { plain.nterms = b.fw.nterms_p; plain.nblk = nblk_p; }
                launch_pair_combine(st, plain, Tf, 1, na, nf, b.ad.nterms, b.ad.nblk, b.d_Btab, b.Upair);
                {
                    ProfScope ps(h, st, CAT_SWEEP, 2.0 * b.k.npad * (double)b.k.npad * cols * m);
                    launch_apply_generators_cols(st, b.k, b.fw, 0, b.Upair, b.EP, 1, m, cols, b.fw.Kpad, (int64_t)Tf * typesz);
                }
                launch_hess_pair(st, h->P, b.k, b.ad, na, b.EP, dH);
            }
        } else if (h->integ_kind[i] == DTO_INTEGRATOR_DERIVATIVE) {
            need_zero();
            launch_hess_derivative(st, h->P, h->der[h->integ_index[i]], dmu, dH);
        } else if (h->integ_kind[i] == DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR) {
            need_zero();
            TdbHost& t = h->tdb[h->integ_index[i]];
            tdb_eval(h, t, dZ, dmu, 2, st);
            launch_extint_hess(st, h->P, t.place, t.d_hess, dH);
        } else {  // the caller's blocks already carry mu_k (eval_hessian_of_lagrangian(integrator, traj, mu_slice))
            need_zero();
            const int e = h->integ_index[i];
            launch_extint_hess(st, h->P, h->ext_int[e], ext_upload(h, e, 2, st), dH);
        }
    }
    need_zero();
    for (auto& c : h->con) {
        if (!c.external) launch_hess_knot(st, h->P, c.k, dZ, dmu, dH);
        else if (c.k.n_times > 0)  // the caller's blocks already carry mu_i (knot_point_constraint.jl:283-291)
            launch_ext_hess(st, h->P, c.xk, 1.0, ext_upload(h, c.ext_slot, 2, st), dH);
    }
    if (sigma != 0.0) {
        // get_full_hessian of the regularizers ASSIGNS its blocks per listed time (regularizers.jl:155-163, :305-309), so a knot
        // listed twice counts once -- unlike their value and gradient, which add per listing (:86-87, :102-108): first layer only
        for (size_t i = 0; i < h->obj.size(); ++i) {
            const bool assigns = h->obj[i].kind == DTO_OBJECTIVE_QUADRATIC_REGULARIZER || h->obj[i].kind == DTO_OBJECTIVE_LINEAR_REGULARIZER;
            for_layers(h, i, [&](const KObj& ol) { launch_hess_objective(st, h->P, ol, dZ, sigma, dH); }, assigns);
        }
        for (auto& e : h->ext_obj)
            if (e.k.n_list > 0) launch_ext_hess(st, h->P, e.k, sigma * e.weight, ext_upload(h, e.ext_slot, 2, st), dH);
    }
}


// ------------------------------------------------------------------------------------------
// host-pointer hand-off plans (dto_hostxfer.h): which slab entries a callback may write a call-dependent value to
// ------------------------------------------------------------------------------------------
void build_jac_plan(dto_handle* h) {
    XferPlan& p = h->jac_plan;
    const KProb& P = h->P;
    const int z = h->z;
    p.total = h->info.jac_len;
    auto var = [&](int64_t at, int64_t n, int64_t early = -1) {
        if (n > 0) { p.start.push_back(at); p.len.push_back(n); p.early.push_back((int32_t)early); }
    };
    auto one = [&](int64_t at, double v) { p.one_pos.push_back(at); p.one_val.push_back(v); };
    // the -E_k block of a lone general-path bilinear integrator is written by the propagator chain alone (do_jacobian): final
    // with its chain chunk
    const bool lone = lone_general_bilinear(h);
    const SlabDims L = slab_dims(h);
    for (int64_t kn = P.kn_lo; kn < P.kn_lo + P.n_knots; ++kn) {
        const bool has_prev = jac_has_part(L, kn, 0), has_own = jac_has_part(L, kn, 1);
        for (int j = 0; j < z; ++j) {
            const int64_t c = kn * z + j;
            const int64_t base = h->colptr[c] - P.jac_lo;
            int pre = 0;
            for (size_t i = 0; i < h->integ_kind.size(); ++i) {
                const int d = h->integ_dim[i];
                const int64_t prev_at = base + jac_part_off(L, kn, pre, d, 0), own_at = base + jac_part_off(L, kn, pre, d, 1);
                const int kind = h->integ_kind[i];
                if (kind == DTO_INTEGRATOR_BILINEAR) {
                    const BilHost& bh = h->bil[h->integ_index[i]];
                    const KBil& b = bh.k;
                    const bool xcol = j >= b.x_off && j < b.x_off + b.n;
                    // z_{k+1} half: identity on the state columns, zeros elsewhere -- constant
                    if (has_prev && xcol) one(prev_at + (j - b.x_off), 1.0);
                    // own rows: -E_k (x), the tangents (u) and -G(u) E_k x (dt) change; every other column is a structural zero
                    // (structured path: of an x column only the rows of its own diagonal block change, the share (r-1)/r of the
                    // x-block is a constant zero -- never shipped, never cleared again in a bound output)
                    if (has_own && bh.kron && xcol) var(own_at + (int64_t)((j - b.x_off) / bh.kb) * bh.kb, bh.kb);
                    else if (has_own && (xcol || (j >= b.u_off && j < b.u_off + b.m) || j == h->dt_idx))
                        var(own_at, d, lone && xcol && j != h->dt_idx && kn - P.kn_lo < P.n_int ? kn - P.kn_lo : -1);
                } else if (kind == DTO_INTEGRATOR_DERIVATIVE) {
                    const KDer& dd = h->der[h->integ_index[i]];
                    const bool xcol = j >= dd.x_off && j < dd.x_off + dd.d, xdcol = j >= dd.xdot_off && j < dd.xdot_off + dd.d;
                    if (has_prev && xcol) one(prev_at + (j - dd.x_off), 1.0);
                    if (has_own) {
                        if (xdcol || j == h->dt_idx) var(own_at, d);         // -dt I and -xdot
                        else if (xcol) one(own_at + (j - dd.x_off), -1.0);   // -I (a column that is x AND xdot / dt is variable)
                    }
                } else {  // host-evaluated and time-dependent bilinear integrators: dense blocks, both halves
                    if (has_prev) var(prev_at, d);
                    if (has_own) var(own_at, d);
                }
                pre += d;
            }
            var(base + jac_con_off(L, kn), h->colptr[c + 1] - h->colptr[c] - jac_con_off(L, kn));  // constraint entries
        }
    }
    if (h->k_hi == h->N) {  // global-variable columns ride with the last knot: constraint entries only
        const int64_t c0 = h->N * z;
        var(h->colptr[c0] - P.jac_lo, h->colptr[h->n_vars] - h->colptr[c0]);
    }
    // the builders above emit per column in ascending order, but a derivative integrator's -1 may precede a later one's runs
    std::vector<size_t> idx(p.one_pos.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return p.one_pos[a] < p.one_pos[b]; });
    std::vector<int64_t> op(idx.size());
    std::vector<double> ov(idx.size());
    for (size_t i = 0; i < idx.size(); ++i) { op[i] = p.one_pos[idx[i]]; ov[i] = p.one_val[idx[i]]; }
    p.one_pos.swap(op);
    p.one_val.swap(ov);
}

void build_hess_plan(dto_handle* h) {
    XferPlan& p = h->hess_plan;
    const KProb& P = h->P;
    const int z = h->z;
    p.total = h->info.hess_len;
    const bool dense_blocks = !h->ext_int.empty() || !h->tdb.empty();  // their 2z x 2z blocks touch everything
    // listed times of the knot terms, per owned knot
    std::vector<std::vector<std::pair<int, int>>> extra((size_t)P.n_knots);  // (a <= b) pairs per local knot
    auto add_pairs = [&](int64_t kn, const std::vector<int32_t>& comps) {
        if (kn < P.kn_lo || kn >= P.kn_lo + P.n_knots) return;
        auto& e = extra[(size_t)(kn - P.kn_lo)];
        for (int a : comps)
            for (int b : comps) e.emplace_back(std::min(a, b), std::max(a, b));
    };
    for (auto& oi : h->obj_info) {
        for (int64_t kn : oi.times) {
            auto& e = extra[(size_t)(kn - P.kn_lo)];
            if (oi.kind == DTO_OBJECTIVE_QUADRATIC_REGULARIZER) {
                for (int c = 0; c < oi.comp_dim; ++c) {
                    const int a = oi.comp_off + c;
                    e.emplace_back(a, a);
                    if (a < h->dt_idx) e.emplace_back(a, h->dt_idx);
                }
                e.emplace_back(h->dt_idx, h->dt_idx);
            } else if (oi.kind == DTO_OBJECTIVE_LINEAR_REGULARIZER) {
                for (int c = 0; c < oi.comp_dim; ++c)
                    if (oi.comp_off + c <= h->dt_idx) e.emplace_back(oi.comp_off + c, h->dt_idx);
            } else if (oi.kind == DTO_OBJECTIVE_KNOT_SQDIST) {
                for (int a : oi.comps) e.emplace_back(a, a);
            } else if (oi.kind == DTO_OBJECTIVE_KNOT_LOWRANK_INFIDELITY) {
                add_pairs(kn, oi.comps);
            }
        }
    }
    for (auto& e : h->ext_obj)
        for (int64_t kn : e.times0) add_pairs(kn, e.comps);
    for (auto& c : h->con)
        if (!c.global)
            for (int64_t kn : c.times0) add_pairs(kn, c.comps);
    const SlabDims L = slab_dims(h);
    std::vector<uint8_t> mask((size_t)z * z);
    auto var = [&](int64_t at, int64_t n) { if (n > 0) { p.start.push_back(at); p.len.push_back(n); } };
    for (int64_t kn = P.kn_lo; kn < P.kn_lo + P.n_knots; ++kn) {
        std::fill(mask.begin(), mask.end(), dense_blocks ? 1 : 0);
        auto set = [&](int a, int b) { mask[(size_t)std::min(a, b) + (size_t)z * std::max(a, b)] = 1; };
        if (!dense_blocks) {
            if (kn < h->K) {
                for (auto& bh : h->bil) {
                    const KBil& b = bh.k;
                    for (int i = 0; i < b.n; ++i) {
                        for (int j = 0; j < b.m; ++j) set(b.x_off + i, b.u_off + j);
                        set(b.x_off + i, h->dt_idx);
                    }
                    for (int i = 0; i < b.m; ++i) {
                        for (int j = 0; j < b.m; ++j) set(b.u_off + i, b.u_off + j);
                        set(b.u_off + i, h->dt_idx);
                    }
                    set(h->dt_idx, h->dt_idx);
                }
                for (auto& dd : h->der)
                    for (int i = 0; i < dd.d; ++i) set(dd.xdot_off + i, h->dt_idx);
            }
            for (auto& ab : extra[(size_t)(kn - P.kn_lo)]) set(ab.first, ab.second);
        }
        const int64_t blk0 = hess_block_start(L, kn) - P.hess_lo;
        for (int b = 0; b < z; ++b) {
            int64_t col = blk0 + hess_col_start(L, kn, b);
            if (dense_blocks) var(col, hess_off_width(L, kn));  // off-diagonal block (kn-1, kn): the cross part of interval kn-1
            col += hess_off_width(L, kn);
            int a = 0;
            while (a <= b) {
                while (a <= b && !mask[(size_t)a + (size_t)z * b]) ++a;
                const int a0 = a;
                while (a <= b && mask[(size_t)a + (size_t)z * b]) ++a;
                var(col + a0, a - a0);
            }
        }
    }
    if (h->k_hi == h->N) var(h->hess_block_nnz - P.hess_lo, (int64_t)h->tail_rows.size());  // global-column tail
}

void build_raw_plans(dto_handle* h) {
    if (h->raw_plans_built) return;
    h->raw_plans_built = true;
    build_jac_plan(h);
    if (h->eval_hessian) build_hess_plan(h);
}

// Bound outputs: the variable runs a callback must clear itself when the full zero-fill is skipped -- every run of the plan except
// the -E_k blocks, which the propagator chain overwrites entry by entry ("early" runs).
bool ensure_bind_runs(dto_handle* h, int which) {
    if (h->bind_ready[which]) return h->n_bind_runs[which] >= 0;
    h->bind_ready[which] = true;
    build_raw_plans(h);
    const XferPlan& p = which == 0 ? h->jac_plan : h->hess_plan;
    h->n_bind_runs[which] = -1;
    if (p.total <= 0) return false;
    std::vector<int64_t> st, ln;
    int64_t var_total = 0;
    for (size_t r = 0; r < p.start.size(); ++r) {
        var_total += p.len[r];
        if (!p.early.empty() && p.early[r] >= 0) continue;
        st.push_back(p.start[r]);
        ln.push_back(p.len[r]);
    }
    if (var_total * 10 > p.total * 9) return false;  // (nearly) everything varies: the plain zero-fill is as good
    h->d_bind_start[which] = own(h, dupload(st));
    h->d_bind_len[which] = own(h, dupload(ln));
    h->n_bind_runs[which] = (int64_t)st.size();
    return true;
}

void ensure_plans(dto_handle* h) {
    if (h->plans_built) return;
    h->plans_built = true;
    if (!h->host_xfer) return;
    build_raw_plans(h);
    for (XferPlan* p : {&h->jac_plan, &h->hess_plan}) {
        if (p->total <= 0) continue;
        p->finalize(h->P.n_int, HostXfer::CHUNK_DOUBLES);
        // shipping the runs pays only when a good part of the slab stays at home
        if (p->packed_total() * 10 > p->total * 9 || p->n_runs() == 0) continue;
        p->d_start = own(h, dupload(p->pk_start));
        p->d_len = own(h, dupload(p->pk_len));
        p->d_poff = own(h, dupload(p->pk_poff));
        p->d_packed = own(h, dalloc<double>((size_t)std::max<int64_t>(p->packed_total(), 1)));
    }
    if (h->jac_plan.usable() || h->hess_plan.usable()) h->xfer.reset(new HostXfer());
}

double* staging(dto_handle* h, size_t n) {
    if (n > h->d_out_cap) {
        h->d_out = own(h, dalloc<double>(n));
        h->d_out_cap = n;
    }
    return h->d_out;
}

void drop_caches(dto_handle* h) {
    invalidate_sweep_caches(h);
    ++h->gen;  // (every kept point: dto_kept_point.h)
}
void unprime(dto_handle* h) { h->primed[0] = h->primed[1] = false; }

// Enqueue, behind the kernels of an asynchronous call, the copy of every sweep's statistics to pinned memory.
void enqueue_stats(dto_handle* h, hipStream_t st) {
    if (!h->h_stats) return;
    size_t i = 0;
    bool any = false;
    for (auto& b : h->bil)
        for (SweepBuf* w : {&b.fw, &b.ad}) {
            if (w->stats) {
                HIP_CHECK(hipMemcpyAsync(h->h_stats + 2 * i, w->stats, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
                any = true;
            }
            ++i;
        }
    if (!any) return;
    HIP_CHECK(hipEventRecord(h->ev_done, st));
    h->stats_pending = true;
}
// Look at the statistics of the last call (waits for them): a sweep that ran out of its step budget is an error.
void check_sweeps(dto_handle* h, bool wait = true) {
    if (!h->stats_pending) return;
    // a call that runs no sweep of its own (objective, gradient) does not wait for the previous asynchronous call: it looks
    // only if that call has finished, and otherwise leaves the check to the next call that would overwrite the statistics
    if (!wait && hipEventQuery(h->ev_done) != hipSuccess) { (void)hipGetLastError(); return; }
    h->stats_pending = false;
    HIP_CHECK(hipEventSynchronize(h->ev_done));
    if (h->smax_pending) { h->last_smax = h->mailbox->deferred_smax; h->smax_pending = false; }
    size_t i = 0;
    bool bad = false;
    for (auto& b : h->bil)
        for (SweepBuf* w : {&b.fw, &b.ad}) {
            if (w->stats) {
                h->last_terms = std::max(h->last_terms, h->h_stats[2 * i + 1]);
                if (h->h_stats[2 * i] != 0) bad = true;
            }
            ++i;
        }
    if (bad) {
        drop_caches(h);  // whatever the sweeps left behind is not a converged result
        throw HipError{"generator sweep did not converge within its step budget"};
    }
}

// Every entry point that evaluates runs through here.  ASYNC: device-pointer form on stream `st` -- device-side errors are
// reported by the NEXT call (check_sweeps at entry); BLOCKING: host-pointer form, checked before it returns; PLAIN: no sweeps.
enum { G_PLAIN = 0, G_ASYNC = 1, G_BLOCKING = 2 };
template <class F>
int guarded(dto_handle* h, F&& f, int mode = G_PLAIN, hipStream_t st = nullptr) {
    if (!h) return fail(nullptr, "null handle");
    if (h->structure_only) return fail(h, "structure-only handle (created with device < 0): no evaluation without a GPU");
    try {
        HIP_CHECK(hipSetDevice(h->device));
        check_sweeps(h, mode != G_PLAIN);  // deferred error of the previous asynchronous call, if any
        (void)hipGetLastError();    // the launches below are judged on their own
        f();
        // kernel launches report a rejected configuration through the runtime's last-error slot, not a return value
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) throw HipError{std::string("kernel launch failed: ") + hipGetErrorString(le)};
        if (mode == G_BLOCKING) { enqueue_stats(h, h->stream); check_sweeps(h); }
        else if (mode == G_ASYNC) enqueue_stats(h, st);
        return 0;
    } catch (const HipError& e) {
        drop_caches(h);
        h->stats_pending = false;
        h->smax_pending = false;
        return fail(h, e.msg);
    } catch (const std::exception& e) {
        drop_caches(h);
        h->stats_pending = false;
        return fail(h, e.what());
    }
}

// ---- multi-GPU: ranges, gather plans, collectives (dto_comm.h)
void set_ranges(dto_handle* h, int rank, int world, const int64_t* k_lo, const int64_t* k_hi) {
    if (world < 1 || rank < 0 || rank >= world) throw HipError{"dto_comm: bad rank / world"};
    std::vector<std::pair<int64_t, int64_t>> rr;
    for (int r = 0; r < world; ++r) {
        if (k_lo[r] < 1 || k_hi[r] < k_lo[r] || k_hi[r] > h->N) throw HipError{"dto_comm: a rank's knot range is out of bounds"};
        rr.emplace_back(k_lo[r], k_hi[r]);
    }
    if (rr[rank].first != h->k_lo || rr[rank].second != h->k_hi)
        throw HipError{"dto_comm: this rank's entry of the knot ranges is not the handle's own shard"};
    std::vector<Slab> sl[3];
    for (int r = 0; r < world; ++r) {
        const ShardExtents e = shard_extents(h, rr[r].first, rr[r].second);
        sl[0].push_back(Slab{e.jac_lo, e.jac_len});
        sl[1].push_back(Slab{e.hess_lo, e.hess_len});
        sl[2].push_back(Slab{e.grad_lo, e.grad_len});
    }
    h->gather_plan[0] = make_gather_plan(sl[0], h->jac_nnz);
    h->gather_plan[1] = make_gather_plan(sl[1], h->hess_nnz);
    h->gather_plan[2] = make_gather_plan(sl[2], h->n_vars);
    h->cons_segments.clear();
    h->cons_segment_root.clear();
    for (int r = 0; r < world; ++r)
        for (auto& sg : shard_row_segments(h, rr[r].first, rr[r].second)) {
            h->cons_segments.push_back(Slab{sg.first, sg.second});
            h->cons_segment_root.push_back(r);
        }
    h->rank_ranges.swap(rr);
    h->comm_rank = rank;
}

const GatherPlan& plan_of(const dto_handle* h, int vector) {
    if (h->rank_ranges.empty()) throw HipError{"no knot ranges yet: dto_comm_create / dto_comm_set_ranges first"};
    if (vector < DTO_VECTOR_JACOBIAN || vector > DTO_VECTOR_GRADIENT) throw HipError{"dto_gather: unknown vector kind"};
    return h->gather_plan[vector - 1];
}

void gather_vector(dto_handle* h, int vector, double* dbuf, hipStream_t st) {
    const GatherPlan& pl = plan_of(h, vector);
    if (!h->comm) throw HipError{"dto_gather: no communicator (dto_comm_create)"};
    if (vector == DTO_VECTOR_HESSIAN && !h->eval_hessian) throw HipError{"handle was created with eval_hessian = 0"};
    std::string e;
    if (pl.in_place) {
        e = h->comm->all_gather_in_place(dbuf, pl.n, st);
    } else {
        std::vector<int> root(pl.slabs.size());
        for (size_t r = 0; r < root.size(); ++r) root[r] = (int)r;
        e = h->comm->broadcast_slabs(dbuf, pl.slabs, root, st);
    }
    if (!e.empty()) throw HipError{e};
}

// the comm entry points touch no sweep state: errors come back at once, nothing is deferred
template <class F>
int comm_guarded(dto_handle* h, F&& f, bool needs_device = true) {
    if (!h) return fail(nullptr, "null handle");
    try {
        if (needs_device) {
            if (h->structure_only) throw HipError{"structure-only handle (created with device < 0): no collectives without a GPU"};
            HIP_CHECK(hipSetDevice(h->device));
        }
        f();
        return 0;
    } catch (const HipError& e) {
        return fail(h, e.msg);
    } catch (const std::exception& e) {
        return fail(h, e.what());
    }
}

// Option "host_xfer_check": the hand-off plans (build_jac_plan / build_hess_plan) are a second statement of which slab entries
// a callback may write; a kernel that writes outside them would be dropped silently on the host-pointer path.  With the
// option on, every such call also copies the WHOLE device slab and compares it bit for bit with what was assembled.
void check_against_slab(dto_handle* h, const double* d_slab, const double* assembled, size_t n, const char* what) {
    std::vector<double> full(n);
    HIP_CHECK(hipMemcpy(full.data(), d_slab, n * sizeof(double), hipMemcpyDeviceToHost));
    if (memcmp(full.data(), assembled, n * sizeof(double)) == 0) return;
    size_t i = 0;
    while (i < n && memcmp(&full[i], &assembled[i], sizeof(double)) == 0) ++i;
    char buf[256];
    snprintf(buf, sizeof(buf), "host_xfer_check: %s entry %zu is %.17g on the device and %.17g in the caller's vector -- a kernel "
             "wrote outside the hand-off plan", what, i, full[i], assembled[i]);
    throw HipError{buf};
}

void upload_Z(dto_handle* h, const double* Z) {
    HIP_CHECK(hipMemcpyAsync(h->d_Z, Z, sizeof(double) * (size_t)h->n_vars, hipMemcpyHostToDevice, h->stream));
}

// ---- Hessian-vector products (dto_eval_hessian_product[_dev], dto_hess_product.hip)

// Walks positions of the unsharded Hessian slab in slab order and names the (row, col) of each, 0-based: the knot blocks
// (HessBlockCursor, dto_slab_layout.h), then the CSC tail of the global-variable columns.
struct HessCursor {
    const dto_handle* h;
    HessBlockCursor blk;
    int64_t j = 0, e = 0;  // past the blocks: entry e of the tail, in global column j
    explicit HessCursor(const dto_handle* h_) : h(h_), blk(slab_dims(h_)) {}
    void tail_col() { while (j < h->gd && e >= h->tail_colptr[(size_t)j + 1]) ++j; }
    void seek(int64_t pos) {
        blk.seek(std::min(pos, h->hess_block_nnz));
        e = std::max<int64_t>(pos - h->hess_block_nnz, 0);
        j = 0;
        if (!blk.in_blocks()) tail_col();
    }
    void next() {
        if (blk.in_blocks()) blk.next(); else ++e;
        if (!blk.in_blocks()) tail_col();
    }
    int64_t row() const { return blk.in_blocks() ? blk.row() : h->tail_rows[(size_t)e]; }
    int64_t col() const { return blk.in_blocks() ? blk.col() : h->N * h->z + j; }
};

// Once per handle, on the host: the row-major copy of both triangles.  Its entries are the slab positions that can be non-zero
// (the Hessian hand-off plan: variable runs and constants, each position once); an off-diagonal position counts for (i, j) and
// (j, i), as MOI defines the product.  Entries are emitted in slab order, which is column-major over the upper triangle, so every
// row of the copy lists its columns in ascending order (a duplicate (i, j) in the tail stays a separate entry, summed in order).
void build_hp_index(dto_handle* h) {
    if (h->hp_index) return;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t nv = h->n_vars;
    if (nv >= ((int64_t)1 << 31)) throw HipError{"Hessian-vector products: n_vars does not fit their 32-bit column indices"};
    build_raw_plans(h);
    const XferPlan& p = h->hess_plan;
    std::vector<std::pair<int64_t, int64_t>> runs;
    for (size_t i = 0; i < p.start.size(); ++i)
        if (p.len[i] > 0) runs.emplace_back(p.start[i], p.len[i]);
    for (int64_t q : p.one_pos) runs.emplace_back(q, 1);
    std::sort(runs.begin(), runs.end());
    auto walk = [&](auto&& emit) {
        HessCursor cur(h);
        int64_t done = 0;  // every position below this one was visited
        for (auto& rl : runs) {
            const int64_t a = std::max(rl.first, done), end = rl.first + rl.second;
            if (a >= end) continue;
            if (a < 0 || end > h->info.hess_len) throw HipError{"Hessian-vector products: hand-off plan outside the slab"};
            cur.seek(a);
            for (int64_t q = a; q < end; ++q, cur.next()) {
                const int64_t row = cur.row(), col = cur.col();
                if (row < 0 || row >= nv || col < 0 || col >= nv) throw HipError{"Hessian-vector products: entry outside the matrix"};
                emit(row, col, q);
            }
            done = end;
        }
    };
    std::vector<int32_t> len((size_t)nv, 0);
    walk([&](int64_t row, int64_t col, int64_t) { ++len[(size_t)row]; if (row != col) ++len[(size_t)col]; });
    std::vector<int64_t> start((size_t)nv);
    int64_t nnz = 0;
    for (int64_t r = 0; r < nv; ++r) {  // every row starts at an even entry (16-byte loads of value pairs)
        start[(size_t)r] = nnz;
        nnz += len[(size_t)r];
        nnz += nnz & 1;
    }
    std::vector<int32_t> col((size_t)std::max<int64_t>(nnz, 2), 0);
    std::vector<int64_t> pos(col.size(), -1);
    std::vector<int64_t> fill(start);
    walk([&](int64_t row, int64_t c, int64_t q) {
        int64_t& a = fill[(size_t)row];
        col[(size_t)a] = (int32_t)c;
        pos[(size_t)a++] = q;
        if (row != c) {
            int64_t& t = fill[(size_t)c];
            col[(size_t)t] = (int32_t)row;
            pos[(size_t)t++] = q;
        }
    });
    // classes of rows by length: 4, 16 or 64 lanes per row
    static const int G[3] = {4, 16, 64};
    auto cls = [](int32_t l) { return l <= 16 ? 0 : l <= 128 ? 1 : 2; };
    std::vector<int32_t> rows;
    rows.reserve((size_t)nv);
    KHessProduct& k = h->hp;
    k = KHessProduct{};
    for (int c = 0; c < 3; ++c) {
        const int64_t r0 = (int64_t)rows.size();
        for (int64_t r = 0; r < nv; ++r)
            if (cls(len[(size_t)r]) == c) rows.push_back((int32_t)r);
        const int64_t nr = (int64_t)rows.size() - r0;
        if (nr == 0) continue;
        const int per = 256 / G[c];
        k.row0[k.n_cls] = r0;
        k.cls_g[k.n_cls] = G[c];
        k.blk0[k.n_cls + 1] = k.blk0[k.n_cls] + (nr + per - 1) / per;
        ++k.n_cls;
        k.row0[k.n_cls] = (int64_t)rows.size();
    }
    k.start = own(h, dupload(start));
    k.len = own(h, dupload(len));
    k.col = own(h, dupload(col));
    k.rows = own(h, dupload(rows));
    h->d_hp_pos = own(h, dupload(pos));
    h->d_hp_val = own(h, dalloc<double>(col.size()));
    k.val = h->d_hp_val;
    h->hp_nnz = (int64_t)col.size();
    alloc_point(h, h->hp_point, true);
    h->hp_index = true;
    h->hp_bytes = 8.0 * (double)h->info.hess_len + (8.0 + 4.0 + 8.0) * (double)h->hp_nnz + (8.0 + 4.0 + 4.0) * (double)nv;
    h->hp_setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// y = H(Z; sigma, mu) v.  At a new point: do_hessian into the private slab, one gather into the row-major copy; at the kept point
// (hp_point: Z, sigma, mu) the product launch alone.
// The Hessian point: the row-major copy at (Z, sigma, mu), rebuilt unless hp_point keeps it.
void hess_point(dto_handle* h, const double* dZ, double sigma, const double* dmu, hipStream_t st) {
    build_hp_index(h);
    if (!at_kept_point(h, h->hp_point, st, dZ, sigma, dmu)) {
        if (!h->hp_slab) h->hp_slab = own(h, dalloc<double>((size_t)h->info.hess_len));
        do_hessian(h, dZ, sigma, dmu, h->hp_slab, st);
        h->hp_slab_primed = true;
        {
            ProfScope ps(h, st, CAT_HESS_PRODUCT, 24.0 * (double)h->hp_nnz);  // position, slab entry, value
            launch_hess_gather(st, h->hp_slab, h->d_hp_pos, h->hp_nnz, h->d_hp_val);
        }
        keep_point(h, h->hp_point, st, dZ, sigma, dmu);
    }
}
void hess_product(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* dv, double* dy, hipStream_t st) {
    hess_point(h, dZ, sigma, dmu, st);
    // bytes: values and columns of every entry, and per row its start, length, id, v and y (v read once: it stays in cache)
    ProfScope ps(h, st, CAT_HESS_PRODUCT, 12.0 * (double)h->hp_nnz + 32.0 * (double)h->n_vars);
    launch_hess_spmv(st, h->hp, dv, dy);
}
// Y = H V for w columns AT the Hessian point (hess_point first): one launch.  Bytes: per tile of columns the values and columns of
// every entry and the rows' start, length and id; per column v and y.
void hess_product_block(dto_handle* h, const KHessBlock& B, const double* dV, double* dY, hipStream_t st) {
    const int T = hess_block_tile(B.w);
    const double tiles = (double)((B.w + T - 1) / T);
    ProfScope ps(h, st, CAT_HESS_PRODUCT, tiles * (12.0 * (double)h->hp_nnz + 16.0 * (double)h->n_vars) + 16.0 * (double)h->n_vars * B.w);
    launch_hess_spmm(st, h->hp, B, dV, dY);
}

void hess_product_applies(const dto_handle* h) {
    if (!h->eval_hessian) throw HipError{"handle was created with eval_hessian = 0"};
    if (h->k_lo != 1 || h->k_hi != h->N) throw HipError{"Hessian-vector products need an unsharded handle"};
}

}  // namespace

// ============================================================================================
// C ABI
// ============================================================================================

extern "C" {

const char* dto_last_error(const dto_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

void dto_destroy(dto_handle* h) { delete h; }

int dto_num_vars(const dto_handle* h, int64_t* out) { if (!h || !out) return 1; *out = h->n_vars; return 0; }
int dto_num_cons(const dto_handle* h, int64_t* out) { if (!h || !out) return 1; *out = h->n_cons; return 0; }
int dto_num_dynamics_cons(const dto_handle* h, int64_t* out) { if (!h || !out) return 1; *out = h->n_dyn; return 0; }
int dto_jac_nnz(const dto_handle* h, int64_t* out) { if (!h || !out) return 1; *out = h->jac_nnz; return 0; }
int dto_hess_nnz(const dto_handle* h, int64_t* out) { if (!h || !out) return 1; *out = h->hess_nnz; return 0; }
int dto_features_available(const dto_handle* h, int32_t* grad, int32_t* jac, int32_t* hess) {
    if (!h) return 1;
    if (grad) *grad = 1;
    if (jac) *jac = 1;
    if (hess) *hess = h->eval_hessian ? 1 : 0;
    return 0;
}
int dto_get_shard_info(const dto_handle* h, dto_shard_info* out) { if (!h || !out) return 1; *out = h->info; return 0; }
int dto_shard_rows(const dto_handle* h, int64_t* start1, int64_t* len) {
    if (!h || !start1 || !len) return 1;
    for (size_t i = 0; i < h->row_segments.size(); ++i) {
        start1[i] = h->row_segments[i].first + 1;
        len[i] = h->row_segments[i].second;
    }
    return 0;
}

// Cost model of one eval_constraint_jacobian per interval ("balanced by sum s_k if scaling counts vary"), host
// arithmetic on Z with the norms of the generators the handle keeps: the same growth bounds the engine plans with (k_norm_bounds:
// b1 >= ||A_k||_1 from ||G_j||_1, b2 >= ||A_k^2||_1^(1/2) from ||G_i G_j||_1 where the handle has them -- a GPU handle), turned into
// squaring counts of the cheaper evaluation form, the Taylor terms of the sweep and their flop counts.
int dto_interval_costs(const dto_handle* h, const double* Z, int64_t first, int64_t count, double* cost) {
    if (!h || !Z || !cost || first < 0 || count < 0 || first + count > h->K) return 1;
    for (int64_t i = 0; i < count; ++i) cost[i] = 0.0;
    for (const BilHost& b : h->bil) {
        if (b.kron) {
            // structured path: one sweep of (1 + m) r + b columns against bp x bp blocks, about two sources per column and term; the
            // norm bound of a block is that of the whole generator (||I (x) B||_1 = ||B||_1)
            const double bp = b.kk.bp, cols = (1.0 + b.k.m) * ((b.kk.rw + 15) / 16 * 16) + bp;
            for (int64_t i = 0; i < count; ++i) {
                const double* zk = Z + (first + i) * h->z;
                double b1 = b.g1[0];
                for (int j = 0; j < b.k.m; ++j) b1 += std::fabs(zk[b.k.u_off + j]) * b.g1[j + 1];
                b1 *= std::fabs(zk[h->dt_idx]);
                if (!(b1 == b1) || b1 > 1e6) b1 = 1e6;
                const SweepPlan sp = plan_sweep(b1);
                cost[i] += 2.0 * bp * bp * cols * 2.0 * (double)sp.d_ub * sp.q;
            }
            continue;
        }
        const int m1 = b.k.m + 1;
        const double np = b.k.npad, gemm = 2.0 * np * np * np;
        // multisets of sizes 2..4 (and 0..4 for the factor K) over m + 1 generators: the generator-subspace GEMMs
        const double c2 = m1 * (m1 + 1) / 2.0, c3 = c2 * (m1 + 2) / 3.0, c4 = c3 * (m1 + 3) / 4.0;
        const double basis = b.small ? 0.0 : 2.0 * np * np * (2.0 * (c2 + c3 + c4) + 1 + m1);
        for (int64_t i = 0; i < count; ++i) {
            const double* zk = Z + (first + i) * h->z;
            const double dt = std::fabs(zk[h->P.dt_idx]);
            double ub[MAX_DRIVES + 1];
            ub[0] = 1.0;
            for (int j = 0; j < b.k.m; ++j) ub[j + 1] = std::fabs(zk[b.k.u_off + j]);
            double b1 = 0.0, s2 = 0.0;
            for (int a = 0; a < m1; ++a) {
                b1 += ub[a] * b.g1[a];
                if ((int)b.n2.size() == m1 * m1)
                    for (int c = 0; c < m1; ++c) s2 += ub[a] * ub[c] * b.n2[a * m1 + c];
            }
            b1 *= dt;
            double alpha = b1;
            if ((int)b.n2.size() == m1 * m1) alpha = std::min(b1, dt * std::sqrt(s2));
            if (!(alpha == alpha) || alpha > 1e6) alpha = 1e6;
            const double sq2 = alpha > THETA_16 ? std::ceil(std::log2(alpha / THETA_16)) : 0.0;
            const double sq3 = alpha > THETA_3P ? std::ceil(std::log2(alpha / THETA_3P)) : 0.0;
            const double products = std::min(2.0 + sq2, 3.0 + sq3);
            const SweepPlan sp = plan_sweep(alpha);
            const double sweep = 2.0 * np * np * m1 * m1 * (double)sp.d_ub * sp.q;
            if (b.follows()) { cost[i] += sweep; continue; }  // its propagators are copies of the leader's: no chain of its own
            cost[i] += b.small ? 2.0 * b.k.n * (double)b.k.n * b.k.n * (6.0 + sq2) : gemm * products + basis + sweep;
        }
    }
    // time-dependent bilinear integrators of 65..256 states: the flops of one Jacobian call of k_tdb_mfma (fixed steps: the same
    // for every interval); an active group by the flops of its launches, counted at its leader
    for (const TdbHost& t : h->tdb)
        if (t.kron || t.mfma) {   // (the structured path by its own flops)
            double c = t.kron ? tdb_kron_flops(t.k, t.kk, 1) : tdb_mfma_flops(t.k, 1);
            if (t.share_active && tdb_share_cap(h, t) >= 2) {
                c = 0.0;
                if (!t.share_members.empty())
                    tdb_share_launches(h, t, [&](int, int n) { c += tdb_mfma_flops(t.k, 1, n); });
            }
            for (int64_t i = 0; i < count; ++i) cost[i] += c;
        }
    // every other term kind costs O(z) per knot: a constant that keeps intervals without a bilinear integrator from counting as free
    for (int64_t i = 0; i < count; ++i) cost[i] += 64.0 * h->z;
    return 0;
}

int dto_integrator_blocks(const dto_handle* h, int32_t integrator, int32_t* block_dim, int32_t* reps, int32_t* active) {
    if (!h || integrator < 0 || integrator >= (int32_t)h->integ_kind.size()) return 1;
    int bd = h->integ_dim[integrator], r = 1, on = 0;
    if (h->integ_kind[integrator] == DTO_INTEGRATOR_BILINEAR) {
        const BilHost& b = h->bil[h->integ_index[integrator]];
        if (b.kr >= 2) { bd = b.kb; r = b.kr; on = b.kron ? 1 : 0; }
    }
    if (h->integ_kind[integrator] == DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR) {
        const TdbHost& t = h->tdb[h->integ_index[integrator]];
        if (t.kr >= 2) { bd = t.kb; r = t.kr; on = t.kron ? 1 : 0; }
    }
    if (block_dim) *block_dim = bd;
    if (reps) *reps = r;
    if (active) *active = on;
    return 0;
}

int dto_integrator_share(const dto_handle* h, int32_t integrator, int32_t* leader, int32_t* group_size, int32_t* active) {
    if (!h || integrator < 0 || integrator >= (int32_t)h->integ_kind.size()) return 1;
    int lead = integrator, size = 1, on = 0;
    if (h->integ_kind[integrator] == DTO_INTEGRATOR_BILINEAR) {
        const BilHost& b = h->bil[h->integ_index[integrator]];
        if (b.share_leader >= 0) { lead = h->bil[b.share_leader].list_pos; size = b.share_size; on = b.share_active ? 1 : 0; }
    }
    if (h->integ_kind[integrator] == DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR) {
        const TdbHost& t = h->tdb[h->integ_index[integrator]];
        if (t.share_leader >= 0) { lead = h->tdb[t.share_leader].list_pos; size = t.share_size; on = t.share_active ? 1 : 0; }
    }
    if (leader) *leader = lead;
    if (group_size) *group_size = size;
    if (active) *active = on;
    return 0;
}

int dto_jacobian_structure(const dto_handle* h, int64_t first, int64_t count, int64_t* rows, int64_t* cols) {
    if (!h || !rows || !cols || first < 0 || count < 0 || first + count > h->jac_nnz) return 1;
    if (count == 0) return 0;
    // column containing `first`
    int64_t c = std::upper_bound(h->colptr.begin(), h->colptr.end(), first) - h->colptr.begin() - 1;
    const SlabDims L = slab_dims(h);
    int64_t written = 0;
    for (; c < h->n_vars && h->colptr[c] < first + count; ++c) {
        const int64_t kn = c / h->z;  // >= N: a global-variable column, NonlinearGlobalConstraint rows only
        auto put = [&](int64_t pos, int64_t row0) {
            if (pos < first || pos >= first + count) return;
            rows[pos - first] = row0 + 1;
            cols[pos - first] = c + 1;
            ++written;
        };
        // integrator rows: for each integrator, interval kn-1 (part 0) then interval kn (part 1)
        int pre = 0;
        for (size_t i = 0; i < h->integ_kind.size(); ++i) {
            const int d = h->integ_dim[i];
            for (int part = 0; part < 2; ++part)
                if (jac_has_part(L, kn, part))
                    for (int r = 0; r < d; ++r)
                        put(h->colptr[c] + jac_part_off(L, kn, pre, d, part) + r, h->integ_row_off[i] + (kn - 1 + part) * d + r);
            pre += d;
        }
        const size_t e0 = con_lower(h, c);
        for (size_t e = e0; e < h->con_cols.size() && h->con_cols[e] == c; ++e)
            put(h->colptr[c] + jac_con_off(L, kn) + (int64_t)(e - e0), h->con_rows[e]);
    }
    return written == count ? 0 : 1;
}

int dto_hessian_structure(const dto_handle* h, int64_t first, int64_t count, int64_t* rows, int64_t* cols) {
    if (!h || !rows || !cols || first < 0 || count < 0 || first + count > h->hess_nnz) return 1;
    if (count == 0) return 0;
    HessCursor cur(h);
    cur.seek(first);
    for (int64_t i = 0; i < count; ++i, cur.next()) {
        rows[i] = cur.row() + 1;
        cols[i] = cur.col() + 1;
    }
    return 0;
}

int dto_constraint_bounds(const dto_handle* h, double* lower, double* upper) {
    if (!h || !lower || !upper) return 1;
    for (int64_t i = 0; i < h->n_cons; ++i) { lower[i] = 0.0; upper[i] = 0.0; }
    for (auto& c : h->con)
        if (!c.equality)
            for (int64_t i = 0; i < c.n_times_total * c.g_dim; ++i) lower[c.row_off + i] = -std::numeric_limits<double>::infinity();
    return 0;
}

int dto_num_external(const dto_handle* h, int32_t* n_integrators, int32_t* n_constraints, int32_t* n_objectives) {
    if (!h) return 1;
    if (n_integrators) *n_integrators = h->n_ext_int;
    if (n_constraints) *n_constraints = h->n_ext_con;
    if (n_objectives) *n_objectives = h->n_ext_obj;
    return 0;
}
int dto_set_external(dto_handle* h, int32_t n, const dto_external_values* v) {
    if (!h) return 1;
    if (n != h->n_ext_int + h->n_ext_con + h->n_ext_obj || (n > 0 && !v))
        return fail(h, "dto_set_external: one entry per external term is required (integrators, constraints, objectives)");
    for (int i = 0; i < n && i < (int)h->ext.size(); ++i) h->ext[i].v = v[i];
    ++h->gen;  // new blocks: the Hessian-vector products' cached point is stale
    return 0;
}

// ---- device-pointer callbacks
int dto_eval_objective_dev(dto_handle* h, const double* dZ, double* df, void* stream) {
    return guarded(h, [&] { do_objective(h, dZ, df, (hipStream_t)stream); });
}
int dto_eval_gradient_dev(dto_handle* h, const double* dZ, double* dgrad, void* stream) {
    return guarded(h, [&] { do_gradient(h, dZ, dgrad, (hipStream_t)stream); });
}
int dto_eval_constraint_dev(dto_handle* h, const double* dZ, double* dg, void* stream) {
    return guarded(h, [&] { do_constraint(h, dZ, dg, (hipStream_t)stream); }, G_ASYNC, (hipStream_t)stream);
}
int dto_eval_jacobian_dev(dto_handle* h, const double* dZ, double* dvals, void* stream) {
    return guarded(h, [&] {
        do_jacobian(h, dZ, dvals, (hipStream_t)stream);
        if (h->bound[0] == dvals) h->primed[0] = true;
    }, G_ASYNC, (hipStream_t)stream);
}
int dto_eval_hessian_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, double* dvals, void* stream) {
    return guarded(h, [&] {
        if (!h->eval_hessian) throw HipError{"handle was created with eval_hessian = 0"};
        do_hessian(h, dZ, sigma, dmu, dvals, (hipStream_t)stream);
        if (h->bound[1] == dvals) h->primed[1] = true;
    }, G_ASYNC, (hipStream_t)stream);
}
int dto_eval_hessian_product_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* dv, double* dy, void* stream) {
    return guarded(h, [&] {
        hess_product_applies(h);
        hess_product(h, dZ, sigma, dmu, dv, dy, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}

// ---- host-pointer callbacks (blocking)
int dto_eval_objective(dto_handle* h, const double* Z, double* f) {
    return guarded(h, [&] {
        upload_Z(h, Z);
        do_objective(h, h->d_Z, h->d_f, h->stream);
        HIP_CHECK(hipMemcpyAsync(f, h->d_f, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}
int dto_eval_gradient(dto_handle* h, const double* Z, double* grad) {
    return guarded(h, [&] {
        upload_Z(h, Z);
        double* o = staging(h, (size_t)h->info.grad_len);
        do_gradient(h, h->d_Z, o, h->stream);
        HIP_CHECK(hipMemcpyAsync(grad, o, sizeof(double) * (size_t)h->info.grad_len, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}
int dto_eval_constraint(dto_handle* h, const double* Z, double* g) {
    return guarded(h, [&] {
        upload_Z(h, Z);
        double* o = staging(h, (size_t)h->cons_len);
        do_constraint(h, h->d_Z, o, h->stream);
        HIP_CHECK(hipMemcpyAsync(g, o, sizeof(double) * (size_t)h->cons_len, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_eval_jacobian(dto_handle* h, const double* Z, double* vals) {
    return guarded(h, [&] {
        upload_Z(h, Z);
        double* o = staging(h, (size_t)h->info.jac_len);
        ensure_plans(h);
        if (h->jac_plan.usable()) {
            // constants are filled by host threads while the GPU computes; only the variable runs cross PCIe, and the -E_k
            // blocks start crossing as soon as their chain chunk is done (dto_hostxfer.h)
            const XferPlan& pl = h->jac_plan;
            h->xfer->begin(pl, o, vals);
            try {
                ChainChunks early;
                if (pl.n_early() > 0) {
                    // from 512 intervals on the chain runs in four chunks (multiples of 8 intervals), each handed over when done
                    const int64_t nint = h->P.n_int;
                    if (nint >= 512) early.cap = (int)(((nint + 3) / 4 + 7) / 8 * 8);
                    early.done = [&](int64_t c0, int nb) {
                        h->xfer->submit(pl.early_off[(size_t)c0], pl.early_off[(size_t)(c0 + nb)], h->stream);
                    };
                }
                do_jacobian(h, h->d_Z, o, h->stream, early);
                h->xfer->submit(pl.n_early(), pl.n_runs(), h->stream);
                h->xfer->finish();
            } catch (...) {
                h->xfer->abort();  // joins the host threads before the error leaves
                throw;
            }
            if (h->xfer_check) check_against_slab(h, o, vals, (size_t)h->info.jac_len, "Jacobian");
            return;
        }
        do_jacobian(h, h->d_Z, o, h->stream);
        HIP_CHECK(hipMemcpyAsync(vals, o, sizeof(double) * (size_t)h->info.jac_len, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_eval_hessian(dto_handle* h, const double* Z, double sigma, const double* mu, double* vals) {
    return guarded(h, [&] {
        if (!h->eval_hessian) throw HipError{"handle was created with eval_hessian = 0"};
        upload_Z(h, Z);
        HIP_CHECK(hipMemcpyAsync(h->d_mu, mu, sizeof(double) * (size_t)h->n_cons, hipMemcpyHostToDevice, h->stream));
        double* o = staging(h, (size_t)h->info.hess_len);
        ensure_plans(h);
        if (h->hess_plan.usable()) {
            const XferPlan& pl = h->hess_plan;
            h->xfer->begin(pl, o, vals);
            try {
                do_hessian(h, h->d_Z, sigma, h->d_mu, o, h->stream);
                h->xfer->submit(0, pl.n_runs(), h->stream);
                h->xfer->finish();
            } catch (...) {
                h->xfer->abort();
                throw;
            }
            if (h->xfer_check) check_against_slab(h, o, vals, (size_t)h->info.hess_len, "Hessian");
            return;
        }
        do_hessian(h, h->d_Z, sigma, h->d_mu, o, h->stream);
        HIP_CHECK(hipMemcpyAsync(vals, o, sizeof(double) * (size_t)h->info.hess_len, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}

// y = H(Z; sigma, mu) v -- MOI.eval_hessian_lagrangian_product
int dto_eval_hessian_product(dto_handle* h, const double* Z, double sigma, const double* mu, const double* v, double* y) {
    return guarded(h, [&] {
        hess_product_applies(h);
        upload_Z(h, Z);
        if (h->n_cons > 0) HIP_CHECK(hipMemcpyAsync(h->d_mu, mu, sizeof(double) * (size_t)h->n_cons, hipMemcpyHostToDevice, h->stream));
        if (!h->d_hp_v) h->d_hp_v = own(h, dalloc<double>((size_t)h->n_vars));
        HIP_CHECK(hipMemcpyAsync(h->d_hp_v, v, sizeof(double) * (size_t)h->n_vars, hipMemcpyHostToDevice, h->stream));
        double* o = staging(h, (size_t)h->n_vars);
        hess_product(h, h->d_Z, sigma, h->d_mu, h->d_hp_v, o, h->stream);
        HIP_CHECK(hipMemcpyAsync(y, o, sizeof(double) * (size_t)h->n_vars, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}

// Matrix-free products: no value slab is formed.  Per bilinear integrator: structured -> k_kron's product modes, small -> k_small's,
// general -> exp(A)w_x rides the forward sweep as an extra column type (J w), exp(A')w_k is an adjoint sweep (J' w).
static void jac_product_matrix_free(dto_handle* h, const double* dZ, const double* dw, double* dy, int transpose, hipStream_t st) {
    const int64_t n_out = transpose ? h->n_vars : h->n_cons;
    HIP_CHECK(hipMemsetAsync(dy, 0, sizeof(double) * (size_t)n_out, st));  // fill!(y, 0), evaluator.jl:416,442
    for (auto& b : h->bil) {
        if (b.kron) { kron_product(h, b, dZ, dw, dy, transpose, st); continue; }
        if (b.small) { small_product(h, b, dZ, dw, dy, transpose, st); continue; }
        if (h->P.n_int <= 0) continue;
        b.cache.products_swept();  // the product sweeps use b.fw with their own column types
        SweepPlan plan = plan_from(h, b, dZ, st);
        SweepTypes ty = make_types(b.k.m, false);
        if (!transpose) {
            const int tw = ty.T;
            ty.t[ty.T++] = TypeDesc{0, {0, 0}, {0, 0}, {0, 0}};  // exp(A) w_x: a second "p" column
            SweepBuf ws = b.fw;
            launch_sweep_init(st, h->P, b.k, ws, ty, dZ, nullptr, 0, plan.q);
            launch_sweep_set_type(st, h->P, b.k, ws, ty.T, tw, dw);
            run_sweep(h, b, b.fw, ty, dZ, nullptr, plan, st, SweepArgs().initialised());   // (above, with w_x as the start of its extra column)
            launch_apply_Gu(st, b.k, b.fw, 0, b.fw.S, b.fw.GY);
            launch_jv_bilinear(st, h->P, b.k, b.fw, tw, dw, dy);
        } else {
            run_sweep(h, b, b.fw, ty, dZ, nullptr, plan, st);
            launch_apply_Gu(st, b.k, b.fw, 0, b.fw.S, b.fw.GY);
            run_sweep(h, b, b.ad, make_types(0, false), dZ, dw, plan, st, SweepArgs().adjoint(CAT_SWEEP));
            launch_jtv_bilinear(st, h->P, b.k, b.fw, b.ad, dw, dy);
        }
    }
    for (auto& t : h->tdb) tdb_product(h, t, dZ, dw, dy, transpose, st);
    for (auto& d : h->der) launch_jv_derivative(st, h->P, d, dZ, dw, dy, transpose);
    for (auto& c : h->con) launch_jv_knot(st, h->P, c.k, dZ, dw, dy, transpose);
}

// Which route a product takes.  The slab route keeps: external integrators, time-dependent integrators unless the option
// "tdb_matrix_free_products" is 1 (every device path of theirs has product modes: k_tdb, k_tdb_mfma and the structured
// k_tdb_kron_product), external constraints (their blocks are placed into the value slab), m + 2 > MAX_TYPES, and a transpose
// product without adjoint buffers on the general path (they exist only with eval_hessian; structured and small integrators need
// none, nor do the time-dependent ones).
static bool jac_product_is_matrix_free(const dto_handle* h, int transpose) {
    bool mfree = h->ext_int.empty() && (h->tdb.empty() || h->tdb_matrix_free_products != 0);
    for (auto& b : h->bil) {
        mfree = mfree && b.k.m + 2 <= MAX_TYPES;
        if (!b.kron && !b.small) mfree = mfree && (transpose == 0 || (h->eval_hessian != 0 && b.ad.S != nullptr));
    }
    for (auto& c : h->con) mfree = mfree && !c.external;
    return mfree;
}

// The handle's private Jacobian value slab (the slab route of the products, the rollout): allocated at the first use
static double* jac_scratch(dto_handle* h) {
    if (!h->d_jac_scratch) h->d_jac_scratch = own(h, dalloc<double>((size_t)h->info.jac_len));
    return h->d_jac_scratch;
}

// The device routine both entry-point families run: everything on `st`, dZ / dw / dy device pointers.
static void jac_product(dto_handle* h, const double* dZ, const double* dw, double* dy, int transpose, hipStream_t st) {
    if (h->k_lo != 1 || h->k_hi != h->N) throw HipError{"Jacobian-vector products need an unsharded handle"};
    if (jac_product_is_matrix_free(h, transpose)) return jac_product_matrix_free(h, dZ, dw, dy, transpose, st);
    if (h->integ_kind.size() > 8) throw HipError{"Jacobian-vector products support at most 8 integrators"};
    const int64_t n_out = transpose ? h->n_vars : h->n_cons;
    jac_scratch(h);
    if (!h->d_conbase) {
        std::vector<int64_t> base((size_t)h->n_vars + 1, 0);
        for (size_t e = 0; e < h->con_cols.size(); ++e) base[(size_t)h->con_cols[e] + 1]++;
        for (int64_t c = 0; c < h->n_vars; ++c) base[(size_t)c + 1] += base[(size_t)c];
        h->d_conbase = own(h, dupload(base));
        h->d_con_rows = own(h, dupload(h->con_rows));
        // the constraint entries once more in ROW order (J w gathers every row in ascending column order: no atomics): per
        // constraint row the columns of its entries and their positions in the value slab
        const int64_t n_con_rows = h->n_cons - h->n_dyn;
        std::vector<int64_t> rptr((size_t)n_con_rows + 1, 0), rcol(h->con_rows.size()), rpos(h->con_rows.size());
        for (size_t e = 0; e < h->con_rows.size(); ++e) rptr[(size_t)(h->con_rows[e] - h->n_dyn) + 1]++;
        for (int64_t r = 0; r < n_con_rows; ++r) rptr[(size_t)r + 1] += rptr[(size_t)r];
        std::vector<int64_t> fill(rptr.begin(), rptr.end() - 1);
        for (size_t e = 0; e < h->con_rows.size(); ++e) {   // CSC order: ascending column, so every row's list ends up ascending too
            const int64_t col = h->con_cols[e], r = h->con_rows[e] - h->n_dyn;
            const int64_t at = fill[(size_t)r]++;
            rcol[(size_t)at] = col;
            rpos[(size_t)at] = con_entry_pos(h, col, (int64_t)e - base[(size_t)col]);
        }
        h->d_crow_ptr = own(h, dupload(rptr));
        h->d_crow_col = own(h, dupload(rcol));
        h->d_crow_pos = own(h, dupload(rpos));
    }
    KIntegTable T{};
    T.n = (int)h->integ_kind.size();
    for (int i = 0; i < T.n; ++i) { T.d[i] = h->integ_dim[i]; T.off[i] = h->integ_row_off[i]; }
    do_jacobian(h, dZ, h->d_jac_scratch, st);   // (external blocks are staged as for dto_eval_jacobian_dev)
    HIP_CHECK(hipMemsetAsync(dy, 0, sizeof(double) * (size_t)n_out, st));  // fill!(y, 0), evaluator.jl:416,442
    if (T.n > 0 || !h->con.empty()) {
        if (transpose) launch_jac_spmv(st, h->P, T, h->d_conbase, h->d_con_rows, h->d_jac_scratch, dw, dy, 1, h->gd);
        else launch_jac_rowgather(st, h->P, T, h->n_cons - h->n_dyn, h->d_crow_ptr, h->d_crow_col, h->d_crow_pos, h->n_dyn, h->d_jac_scratch, dw, dy);
    }
}
// host-pointer form: upload, the device routine, download
static void jac_product_host(dto_handle* h, const double* Z, const double* w, double* y, int transpose) {
    const int64_t n_in = transpose ? h->n_cons : h->n_vars, n_out = transpose ? h->n_vars : h->n_cons;
    if (!h->d_w) h->d_w = own(h, dalloc<double>((size_t)std::max(h->n_vars, h->n_cons)));
    upload_Z(h, Z);
    HIP_CHECK(hipMemcpyAsync(h->d_w, w, sizeof(double) * (size_t)n_in, hipMemcpyHostToDevice, h->stream));
    double* o = staging(h, (size_t)n_out);
    jac_product(h, h->d_Z, h->d_w, o, transpose, h->stream);
    HIP_CHECK(hipMemcpyAsync(y, o, sizeof(double) * (size_t)n_out, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
}
// y = J(Z) w  -- MOI.eval_constraint_jacobian_product (evaluator.jl:406-430)
int dto_eval_jacobian_product(dto_handle* h, const double* Z, const double* w, double* y) {
    return guarded(h, [&] { jac_product_host(h, Z, w, y, 0); }, G_BLOCKING);
}
// y = J(Z)' w -- MOI.eval_constraint_jacobian_transpose_product (evaluator.jl:432-456)
int dto_eval_jacobian_transpose_product(dto_handle* h, const double* Z, const double* w, double* y) {
    return guarded(h, [&] { jac_product_host(h, Z, w, y, 1); }, G_BLOCKING);
}
// ... and their device-pointer forms: enqueued on the caller's stream, errors deferred (dto_engine.h, error convention)
int dto_eval_jacobian_product_dev(dto_handle* h, const double* dZ, const double* dw, double* dy, void* stream) {
    return guarded(h, [&] { jac_product(h, dZ, dw, dy, 0, (hipStream_t)stream); }, G_ASYNC, (hipStream_t)stream);
}
int dto_eval_jacobian_transpose_product_dev(dto_handle* h, const double* dZ, const double* dw, double* dy, void* stream) {
    return guarded(h, [&] { jac_product(h, dZ, dw, dy, 1, (hipStream_t)stream); }, G_ASYNC, (hipStream_t)stream);
}

// ---- open-loop rollout: X_{k+1} = E_k(Z) X_k through every interval (dto_rollout.hip, dto_rollout_plan.h)

// grow-only device workspace: a failed allocation throws and leaves the old buffer in place
static double* grow_workspace(dto_handle* h, Workspace& w, size_t doubles) {
    if (doubles <= w.cap && w.p) return w.p;
    double* q = dalloc<double>(doubles);
    if (w.p) {
        h->owned.erase(std::find(h->owned.begin(), h->owned.end(), (void*)w.p));
        (void)hipFree(w.p);   // (waits for whatever still reads it)
    }
    w.p = own(h, q);
    w.cap = doubles;
    return w.p;
}

static void needs_unsharded(const dto_handle* h, const std::string& who) {   // the rollout, the solves and the reduced operators
    if (h->k_lo != 1 || h->k_hi != h->N) throw HipError{who + " needs an unsharded handle (k_lo, k_hi = the whole trajectory)"};
}

// What a rollout call names: refused with text before anything is enqueued.  Returns the kernels' record of the integrator.
static KRollout rollout_args(const dto_handle* h, int32_t integrator, int32_t n_cols, int32_t mode, bool has_X0, const char* who_ = "dto_rollout") {
    const std::string who(who_);
    needs_unsharded(h, who);
    if (integrator < 0 || integrator >= (int32_t)h->integ_kind.size())
        throw HipError{who + ": integrator " + std::to_string(integrator) + " is out of range (the handle has " +
                       std::to_string(h->integ_kind.size()) + ")"};
    if (mode != DTO_ROLLOUT_ALL && mode != DTO_ROLLOUT_FINAL) throw HipError{who + ": mode takes DTO_ROLLOUT_ALL (0) or DTO_ROLLOUT_FINAL (1)"};
    int32_t n = 0, x_off = 0, pre = 0;
    const int kind = h->integ_kind[integrator], idx = h->integ_index[integrator];
    if (kind == DTO_INTEGRATOR_BILINEAR) {
        const KBil& k = h->bil[idx].k;
        n = k.n; x_off = k.x_off; pre = k.pre;
    } else if (kind == DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR) {
        const TdbHost& t = h->tdb[idx];
        n = t.k.n; x_off = t.k.x_off; pre = t.place.pre;
    } else if (kind == DTO_INTEGRATOR_DERIVATIVE) {
        throw HipError{who + ": integrator " + std::to_string(integrator) + " is a DerivativeIntegrator: it has no propagator"};
    } else {
        throw HipError{who + ": integrator " + std::to_string(integrator) + " is evaluated on the host (DTO_INTEGRATOR_EXTERNAL): its "
                       "Jacobian block is not known to be a propagator"};
    }
    if (n_cols < 1 || n_cols > n)
        throw HipError{who + ": n_cols = " + std::to_string(n_cols) + ", allowed 1 .. x_dim = " + std::to_string(n)};
    if (!has_X0 && n_cols != 1) throw HipError{who + ": X0 = NULL (the state of knot 1 of Z) takes n_cols = 1"};
    return KRollout(n, x_off, pre, n_cols, h->K);
}

// Leaves and up-sweep: the product tree of R's integrator from the -E_k blocks of a Jacobian value slab, into `tree`.  The launches
// count under `cat_gather` and `cat_tree`.
static void rollout_tree_from_slab(dto_handle* h, const KRollout& R, const double* slab, double* tree, hipStream_t st, int cat_gather, int cat_tree) {
    const int npad = R.npad, L = R.L;
    const size_t nn = (size_t)npad * npad;
    { ProfScope ps(h, st, cat_gather, 0.0); launch_rollout_leaves(st, h->P, R, slab, tree); }
    // up-sweep: level l + 1 = (second half of level l) * (first half), one contiguous batch
    for (int l = 0; l < L; ++l) {
        const int nb = (int)rollout_level_len(L, l + 1);
        const double* lo = tree + (size_t)rollout_level_off(L, l) * nn;
        ProfScope ps(h, st, cat_tree, 2.0 * npad * (double)nn * nb);
        launch_bgemm_plain(st, npad, nb, lo + (size_t)nb * nn, lo, tree + (size_t)rollout_level_off(L, l + 1) * nn);
    }
}

// Jacobian, gather and up-sweep, for the rollout and the single-integrator solves alike: the product tree of R's integrator at dZ, in
// d_roll_tree.
static double* build_rollout_tree(dto_handle* h, const KRollout& R, const double* dZ, hipStream_t st, int cat_gather, int cat_tree) {
    double* tree = grow_workspace(h, h->d_roll_tree, rollout_tree_bytes(R.npad, R.K) / sizeof(double));
    double* slab = jac_scratch(h);
    // the whole Jacobian, tangent sweep included: the x_k columns of the integrator then hold -E_k on every path
    do_jacobian(h, dZ, slab, st);   // (external blocks are staged as for dto_eval_jacobian_dev)
    rollout_tree_from_slab(h, R, slab, tree, st, cat_gather, cat_tree);
    return tree;
}

// The device routine both entry-point families run: everything on `st`, dZ / dX0 / dX device pointers.
static void rollout(dto_handle* h, const KRollout& R, const double* dZ, const double* dX0, int mode, double* dX, hipStream_t st) {
    const int npad = R.npad, L = R.L;
    const int64_t K = R.K;
    const size_t nn = (size_t)npad * npad;
    double* S = grow_workspace(h, h->d_roll_S, rollout_traj_bytes(npad, K, R.n_cols) / sizeof(double));
    if (K < 1) {   // a single knot: the rollout is X0
        ProfScope ps(h, st, CAT_ROLLOUT_DESCENT, 0.0);
        launch_rollout_start(st, R, dZ, dX0, S);
        launch_rollout_compact(st, R, 0, 1, S, dX);
        return;
    }
    h->dyn_point.rec.drop();   // (the tree the solves keep per point is overwritten)
    double* tree = build_rollout_tree(h, R, dZ, st, CAT_ROLLOUT, CAT_ROLLOUT_TREE);
    { ProfScope ps(h, st, CAT_ROLLOUT_DESCENT, 0.0); launch_rollout_start(st, R, dZ, dX0, S); }
    const double item_flops = 2.0 * (double)nn * R.col_pad;
    if (mode == DTO_ROLLOUT_ALL) {
        for (int l = L + 1; l >= 1; --l) {
            const int64_t live = l == L + 1 ? (K == ((int64_t)1 << L) ? 1 : 0) : (((K >> (l - 1)) + 1) >> 1);
            if (live == 0) continue;
            ProfScope ps(h, st, CAT_ROLLOUT_DESCENT, item_flops * (double)live);
            launch_rollout_descend(st, R, l, -1, tree, S);
        }
        ProfScope ps(h, st, CAT_ROLLOUT_DESCENT, 0.0);
        launch_rollout_compact(st, R, 0, K + 1, S, dX);
    } else {
        // the final state alone: the items on the way from knot K back to knot 0, highest level first -- the same launches on the
        // same operands as in the full descent, so the same bits
        int lv[ROLLOUT_MAX_PATH];
        int64_t ix[ROLLOUT_MAX_PATH];
        for (int c = 0, cnt = rollout_final_path(L, K, lv, ix); c < cnt; ++c) {
            ProfScope ps(h, st, CAT_ROLLOUT_DESCENT, item_flops);
            launch_rollout_descend(st, R, lv[c], ix[c], tree, S);
        }
        ProfScope ps(h, st, CAT_ROLLOUT_DESCENT, 0.0);
        launch_rollout_compact(st, R, K, 1, S, dX);
    }
}

int dto_rollout(dto_handle* h, int32_t integrator, const double* Z, const double* X0, int32_t n_cols, int32_t mode, double* X) {
    return guarded(h, [&] {
        const KRollout R = rollout_args(h, integrator, n_cols, mode, X0 != nullptr);
        upload_Z(h, Z);
        const double* dX0 = nullptr;
        if (X0) {
            double* d = grow_workspace(h, h->d_roll_X0, (size_t)R.n * R.n_cols);
            HIP_CHECK(hipMemcpyAsync(d, X0, sizeof(double) * (size_t)R.n * R.n_cols, hipMemcpyHostToDevice, h->stream));
            dX0 = d;
        }
        const size_t n_out = (size_t)(mode == DTO_ROLLOUT_ALL ? h->N : 1) * R.n_cols * R.n;
        double* o = staging(h, n_out);
        rollout(h, R, h->d_Z, dX0, mode, o, h->stream);
        HIP_CHECK(hipMemcpyAsync(X, o, sizeof(double) * n_out, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_rollout_dev(dto_handle* h, int32_t integrator, const double* dZ, const double* dX0, int32_t n_cols, int32_t mode,
                    double* dX, void* stream) {
    return guarded(h, [&] {
        const KRollout R = rollout_args(h, integrator, n_cols, mode, dX0 != nullptr);
        rollout(h, R, dZ, dX0, mode, dX, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}

// ---- solves with the dynamics block: M Y = B (Y_{k+1} = E_k Y_k + B_{k+1}) and M' Lam = B (Lam_k = E_k' Lam_{k+1} + B_k), affine
// scans over the rollout's tree (dto_dynsolve.hip, dto_rollout_plan.h)

static KRollout dynsolve_args(const dto_handle* h, int32_t integrator, int32_t direction, const double* B, int32_t n_cols, int32_t mode) {
    const KRollout R = rollout_args(h, integrator, n_cols, mode, true, "dto_dynamics_solve");
    if (direction != DTO_SOLVE_FORWARD && direction != DTO_SOLVE_ADJOINT)
        throw HipError{"dto_dynamics_solve: direction takes DTO_SOLVE_FORWARD (0) or DTO_SOLVE_ADJOINT (1)"};
    if (!B) throw HipError{"dto_dynamics_solve: B = NULL (the right-hand side [N][n_cols][x_dim] is required)"};
    return R;
}

// The scan's two halves, for the single-integrator solves and the whole-dynamics solves alike (every launch counts under
// "dynsolve_scan"): the loader with the offsets' up-sweep, and the full descent with the copy into the caller's layout.
static void dynsolve_load_and_up(dto_handle* h, const KRollout& R, int adjoint, const double* tree, const double* dB, double* off, double* S,
                                 hipStream_t st) {
    { ProfScope ps(h, st, CAT_DYNSOLVE_SCAN, 0.0); launch_dynsolve_load(st, R, adjoint, dB, off, S); }
    const double item_flops = 2.0 * (double)R.npad * R.npad * R.col_pad;
    for (int l = 0; l < R.L; ++l) {
        ProfScope ps(h, st, CAT_DYNSOLVE_SCAN, item_flops * (double)rollout_level_len(R.L, l + 1));
        launch_dynsolve_up(st, R, adjoint, l, tree, off);
    }
}
static void dynsolve_descend_all(dto_handle* h, const KRollout& R, int adjoint, const double* tree, double* off, double* S, double* dY,
                                 hipStream_t st) {
    const double item_flops = 2.0 * (double)R.npad * R.npad * R.col_pad;
    for (int l = R.L + 1; l >= 1; --l) {
        if (dynsolve_live_items(R.L, R.K, adjoint, l) == 0) continue;
        ProfScope ps(h, st, CAT_DYNSOLVE_SCAN, item_flops * (double)dynsolve_product_items(R.L, R.K, adjoint, l));
        launch_dynsolve_descend(st, R, adjoint, l, -1, tree, off, S);
    }
    ProfScope ps(h, st, CAT_DYNSOLVE_SCAN, 0.0);
    launch_rollout_compact(st, R, 0, R.K + 1, S, dY);
}

// The device routine both entry-point families run: everything on `st`, dZ / dB / dY device pointers.  The tree is rebuilt (do_jacobian
// into the private slab, leaves, products) unless the one in d_roll_tree is the kept point's (dyn_point: integrator, Z; no rollout since).
static void dynamics_solve(dto_handle* h, const KRollout& R, int32_t integrator, const double* dZ, int adjoint, const double* dB, int mode,
                           double* dY, hipStream_t st) {
    const int npad = R.npad, L = R.L;
    const int64_t K = R.K;
    if (K < 1) {   // a single knot: M is the identity
        ProfScope ps(h, st, CAT_DYNSOLVE_SCAN, 0.0);
        HIP_CHECK(hipMemcpyAsync(dY, dB, sizeof(double) * (size_t)R.n_cols * R.n, hipMemcpyDeviceToDevice, st));
        return;
    }
    double* S = grow_workspace(h, h->d_roll_S, rollout_traj_bytes(npad, K, R.n_cols) / sizeof(double));
    double* off = grow_workspace(h, h->d_dyn_off, dynsolve_offset_bytes(npad, K, R.n_cols) / sizeof(double));
    alloc_point(h, h->dyn_point, false);
    if (!at_kept_point(h, h->dyn_point, st, dZ, 0.0, nullptr, integrator)) {
        build_rollout_tree(h, R, dZ, st, CAT_DYNSOLVE_TREE, CAT_DYNSOLVE_TREE);
        keep_point(h, h->dyn_point, st, dZ, 0.0, nullptr, integrator);
    }
    const double* tree = h->d_roll_tree.p;
    dynsolve_load_and_up(h, R, adjoint, tree, dB, off, S, st);
    const double item_flops = 2.0 * (double)npad * npad * R.col_pad;
    if (mode == DTO_ROLLOUT_ALL) {
        dynsolve_descend_all(h, R, adjoint, tree, off, S, dY, st);
    } else if (adjoint) {
        // knot 1 alone: the root's item -- the same launch on the same operands as in the full descent, so the same bits
        {
            ProfScope ps(h, st, CAT_DYNSOLVE_SCAN, item_flops * (double)dynsolve_product_items(L, K, 1, L + 1));
            launch_dynsolve_descend(st, R, 1, L + 1, 0, tree, off, S);
        }
        ProfScope ps(h, st, CAT_DYNSOLVE_SCAN, 0.0);
        launch_rollout_compact(st, R, 0, 1, S, dY);
    } else {
        // knot N alone: the items on the way from knot K back to knot 0, highest level first, as dto_rollout's final mode runs them
        int lv[ROLLOUT_MAX_PATH];
        int64_t ix[ROLLOUT_MAX_PATH];
        for (int c = 0, cnt = rollout_final_path(L, K, lv, ix); c < cnt; ++c) {
            ProfScope ps(h, st, CAT_DYNSOLVE_SCAN, item_flops);
            launch_dynsolve_descend(st, R, 0, lv[c], ix[c], tree, off, S);
        }
        ProfScope ps(h, st, CAT_DYNSOLVE_SCAN, 0.0);
        launch_rollout_compact(st, R, K, 1, S, dY);
    }
}

int dto_dynamics_solve(dto_handle* h, int32_t integrator, const double* Z, int32_t direction, const double* B, int32_t n_cols, int32_t mode,
                       double* Y) {
    return guarded(h, [&] {
        const KRollout R = dynsolve_args(h, integrator, direction, B, n_cols, mode);
        upload_Z(h, Z);
        const size_t n_in = (size_t)h->N * R.n_cols * R.n;
        double* dB = grow_workspace(h, h->d_dyn_B, n_in);
        HIP_CHECK(hipMemcpyAsync(dB, B, sizeof(double) * n_in, hipMemcpyHostToDevice, h->stream));
        const size_t n_out = (size_t)(mode == DTO_ROLLOUT_ALL ? h->N : 1) * R.n_cols * R.n;
        double* o = staging(h, n_out);
        dynamics_solve(h, R, integrator, h->d_Z, direction == DTO_SOLVE_ADJOINT, dB, mode, o, h->stream);
        HIP_CHECK(hipMemcpyAsync(Y, o, sizeof(double) * n_out, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_dynamics_solve_dev(dto_handle* h, int32_t integrator, const double* dZ, int32_t direction, const double* dB, int32_t n_cols,
                           int32_t mode, double* dY, void* stream) {
    return guarded(h, [&] {
        const KRollout R = dynsolve_args(h, integrator, direction, dB, n_cols, mode);
        dynamics_solve(h, R, integrator, dZ, direction == DTO_SOLVE_ADJOINT, dB, mode, dY, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}

// ---- whole-dynamics solves: the Jacobian block of ALL integrators' rows and state columns, by block elimination in dependency order
// (dto_elim.hip, dto_elim_plan.h).  Each integrator's own block is solved as above -- an affine scan over a tree of its own, or the
// DerivativeIntegrator's serial sum -- after the coupling blocks have carried the finished slices into its right-hand side.

// The plan, from what dto_create kept on the host (a structure-only handle has it too).  A handle with a host-evaluated integrator
// gets a plan that holds only the refusal.
static std::vector<ElimIntegrator> elim_integrators(const dto_handle* h, std::string& external) {
    std::vector<ElimIntegrator> its;
    for (size_t i = 0; i < h->integ_kind.size(); ++i) {
        const int kind = h->integ_kind[i], idx = h->integ_index[i];
        if (kind == DTO_INTEGRATOR_BILINEAR) {
            const KBil& k = h->bil[idx].k;
            its.push_back(ElimIntegrator{ELIM_BILINEAR, k.x_off, k.n, k.u_off, k.m, -1});
        } else if (kind == DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR) {
            const KTdb& k = h->tdb[idx].k;
            its.push_back(ElimIntegrator{ELIM_TIME_DEPENDENT, k.x_off, k.n, k.u_off, k.m, k.t_off});
        } else if (kind == DTO_INTEGRATOR_DERIVATIVE) {
            const KDer& k = h->der[idx];
            its.push_back(ElimIntegrator{ELIM_DERIVATIVE, k.x_off, k.d, k.xdot_off, k.d, -1});
        } else if (external.empty()) {
            external = "integrator " + std::to_string(i) + " is evaluated on the host (DTO_INTEGRATOR_EXTERNAL): its Jacobian block is "
                       "not known to be a propagator";
        }
    }
    return its;
}
static const ElimPlan& elim_plan_of(dto_handle* h) {
    if (h->elim) return *h->elim;
    std::string external;
    const std::vector<ElimIntegrator> its = elim_integrators(h, external);
    std::unique_ptr<ElimPlan> p(new ElimPlan);
    if (external.empty()) *p = elim_plan(its, h->dt_idx, h->K);
    else p->refusal = external;
    h->elim = std::move(p);
    return *h->elim;
}

static bool elim_has_tree(const dto_handle* h, int i) { return h->integ_kind[i] != DTO_INTEGRATOR_DERIVATIVE; }
// first state component of integrator i (a device kind: the plan refuses the others)
static int elim_x_off(const dto_handle* h, int i) {
    const int idx = h->integ_index[i], kind = h->integ_kind[i];
    return kind == DTO_INTEGRATOR_BILINEAR ? h->bil[idx].k.x_off : kind == DTO_INTEGRATOR_DERIVATIVE ? h->der[idx].x_off : h->tdb[idx].k.x_off;
}

// the block solve's record of integrator i (bilinear or time-dependent)
static KRollout elim_rollout_args(const dto_handle* h, const ElimPlan& p, int i, int n_cols) {
    return KRollout(h->integ_dim[i], elim_x_off(h, i), p.pre[i], n_cols, h->K);
}

// each block solve's own limit on n_cols: the smallest x_dim among the integrators with a propagator, 64 without one
static int elim_column_cap(const dto_handle* h) {
    int cap = 0;
    for (size_t i = 0; i < h->integ_kind.size(); ++i)
        if (elim_has_tree(h, (int)i)) cap = cap ? std::min(cap, h->integ_dim[i]) : h->integ_dim[i];
    return cap ? cap : 64;
}

// What a whole-dynamics solve names: refused with text before anything is enqueued.
static const ElimPlan& elim_args(dto_handle* h, int32_t direction, const double* B, int32_t n_cols) {
    const std::string who = "dto_dynamics_solve_all";
    needs_unsharded(h, who);
    const ElimPlan& p = elim_plan_of(h);
    if (!p.refusal.empty()) throw HipError{who + ": " + p.refusal};
    if (direction != DTO_SOLVE_FORWARD && direction != DTO_SOLVE_ADJOINT)
        throw HipError{who + ": direction takes DTO_SOLVE_FORWARD (0) or DTO_SOLVE_ADJOINT (1)"};
    if (!B) throw HipError{who + ": B = NULL (the right-hand side [N][n_cols][n_states] is required)"};
    const int cap = elim_column_cap(h);
    if (n_cols < 1 || n_cols > cap) throw HipError{who + ": n_cols = " + std::to_string(n_cols) + ", allowed 1 .. " + std::to_string(cap)};
    return p;
}

// the contractions' term tables: per integrator its dependencies (forward) and its dependents (adjoint), once per handle
static void elim_upload_terms(dto_handle* h, const ElimPlan& p) {
    if (h->d_elim_terms) return;
    const int I = (int)p.pre.size();
    std::vector<KElimTerm> terms;
    h->elim_fw_term0.assign(1, 0);
    for (int a = 0; a < I; ++a) {
        for (const ElimDep& d : p.deps[a])
            terms.push_back(KElimTerm{p.store_off[a], p.width[a], h->integ_dim[a], d.col, p.pre[d.b], h->integ_dim[d.b]});
        h->elim_fw_term0.push_back((int)terms.size());
    }
    h->elim_ad_term0.assign(1, (int)terms.size());
    for (int a = 0; a < I; ++a) {
        for (int b : p.dependents[a])
            for (const ElimDep& d : p.deps[b])
                if (d.b == a) terms.push_back(KElimTerm{p.store_off[b], p.width[b], h->integ_dim[b], d.col, p.pre[b], h->integ_dim[b]});
        h->elim_ad_term0.push_back((int)terms.size());
    }
    h->d_elim_terms = own(h, dupload(terms));
}

// The device routine both entry-point families run: everything on `st`, dZ / dB / dY device pointers, dB and dY [N][n_cols][D].  At a
// new point: ONE do_jacobian into the private slab, then per integrator with a propagator the leaves and products of its own tree,
// the gather of every coupling block (with the option "reduced_input_store" of every input block too).  At the kept point: none of it.
// dynamics_solve_all = elim_point (workspaces, point check, rebuild) + elim_solve (the block elimination at the kept point).  The
// reduced-space operators' input-store route calls the halves itself: its first kernel reads what the rebuild gathers.
struct ElimWork { double *Bp, *Yp, *S, *off, *store; };

// the input-block store's plan and device tables (option "reduced_input_store"), once per handle
static const InputPlan& input_plan_of(dto_handle* h, const ElimPlan& p) {
    if (h->input) return *h->input;
    std::string external;
    const std::vector<ElimIntegrator> its = elim_integrators(h, external);
    std::unique_ptr<InputPlan> ip(new InputPlan(input_plan(its, h->dt_idx, h->z, h->K)));
    const int I = (int)its.size();
    std::vector<KInputInt> integ;
    std::vector<int32_t> fin, pos_int((size_t)p.n_states, 0), term0(1, 0), read;
    std::vector<KInputTerm> terms;
    for (int a = 0; a < I; ++a) {
        integ.push_back(KInputInt{ip->store_off[a], p.pre[a], its[a].x_dim, ip->width[a], (int32_t)fin.size()});
        fin.insert(fin.end(), ip->fin[a].begin(), ip->fin[a].end());
        for (int r = 0; r < its[a].x_dim; ++r) pos_int[(size_t)(p.pre[a] + r)] = a;
    }
    for (int c = 0; c < h->z; ++c) {
        for (const InputTerm& t : ip->terms[c]) terms.push_back(KInputTerm{ip->store_off[t.a], ip->width[t.a], its[t.a].x_dim, t.j, p.pre[t.a]});
        term0.push_back((int32_t)terms.size());
        if (!ip->terms[c].empty()) read.push_back(c);
    }
    KInput in{};
    in.integ = own(h, dupload(integ));
    in.fin = own(h, dupload(fin));
    in.pos_int = own(h, dupload(pos_int));
    in.term0 = own(h, dupload(term0));
    in.terms = own(h, dupload(terms));
    in.read = own(h, dupload(read));
    in.n_read = (int32_t)read.size();
    in.n_int = I;
    in.K = h->K;
    h->in = in;
    h->input = std::move(ip);
    return *h->input;
}

static ElimWork elim_point(dto_handle* h, const ElimPlan& p, const double* dZ, int n_cols, hipStream_t st) {
    const int I = (int)p.pre.size();
    const int64_t K = h->K, N = h->N;
    // every workspace first: a failed allocation is refused before anything is enqueued
    int n_max = 1, npad_max = 0;
    for (int i = 0; i < I; ++i) {
        n_max = std::max(n_max, h->integ_dim[i]);
        if (elim_has_tree(h, i)) npad_max = std::max(npad_max, pad64(h->integ_dim[i]));
    }
    double* Bp = grow_workspace(h, h->d_elim_Bp, (size_t)N * n_cols * n_max);
    double* Yp = grow_workspace(h, h->d_elim_Yp, (size_t)N * n_cols * n_max);
    double *S = nullptr, *off = nullptr;
    if (npad_max) {
        S = grow_workspace(h, h->d_roll_S, rollout_traj_bytes(npad_max, K, n_cols) / sizeof(double));
        off = grow_workspace(h, h->d_dyn_off, dynsolve_offset_bytes(npad_max, K, n_cols) / sizeof(double));
    }
    double* store = grow_workspace(h, h->d_elim_store, (size_t)p.store_off[I]);
    const InputPlan* ip = h->reduced_input_store ? &input_plan_of(h, p) : nullptr;
    if (ip) grow_workspace(h, h->d_in_store, (size_t)ip->store_off[I]);
    h->elim_tree.resize(I);
    for (int i = 0; i < I; ++i)
        if (elim_has_tree(h, i))
            grow_workspace(h, h->elim_tree[i], rollout_tree_bytes(pad64(h->integ_dim[i]), K) / sizeof(double));
    elim_upload_terms(h, p);
    alloc_point(h, h->elim_point, false);
    if (!at_kept_point(h, h->elim_point, st, dZ)) {
        double* slab = jac_scratch(h);
        do_jacobian(h, dZ, slab, st);   // once, however many integrators there are
        for (int i = 0; i < I; ++i)
            if (elim_has_tree(h, i))
                rollout_tree_from_slab(h, elim_rollout_args(h, p, i, n_cols), slab, h->elim_tree[i].p, st, CAT_DYNSOLVE_TREE, CAT_DYNSOLVE_TREE);
        for (int a = 0; a < I; ++a)
            for (const ElimDep& d : p.deps[a]) {
                const int n_a = h->integ_dim[a], n_b = h->integ_dim[d.b];
                ProfScope ps(h, st, CAT_DYNSOLVE_COUPLE, 16.0 * (double)K * 2.0 * n_a * n_b);
                launch_elim_gather(st, h->P, KElimPair{n_a, p.pre[a], elim_x_off(h, d.b), n_b, d.col, p.width[a]}, K, slab, store + p.store_off[a]);
            }
        if (ip)   // the input blocks sit beside the coupling blocks, in the same knot columns of the same slab
            for (int a = 0; a < I; ++a)
                if (ip->width[a] > 0) {
                    ProfScope ps(h, st, CAT_REDUCED_INPUT, 16.0 * (double)K * 2.0 * ip->width[a] * h->integ_dim[a]);
                    launch_red_input_gather(st, h->P, h->in, a, slab, h->d_in_store.p);
                }
        keep_point(h, h->elim_point, st, dZ);
    }
    return ElimWork{Bp, Yp, S, off, store};
}

static void elim_solve(dto_handle* h, const ElimPlan& p, const ElimWork& W, int adjoint, const double* dB, int n_cols, double* dY, hipStream_t st) {
    const int I = (int)p.pre.size(), D = p.n_states;
    const int64_t K = h->K, N = h->N;
    double *Bp = W.Bp, *Yp = W.Yp, *S = W.S, *off = W.off, *store = W.store;
    for (int step = 0; step < I; ++step) {
        const int a = p.order[adjoint ? I - 1 - step : step], n_a = h->integ_dim[a];
        const std::vector<int>& t0 = adjoint ? h->elim_ad_term0 : h->elim_fw_term0;
        KElimCouple C{n_a, p.pre[a], D, n_cols, t0[a + 1] - t0[a], K, h->d_elim_terms + t0[a]};
        {
            // bytes: B in, Bp out, and per term both halves of the store's columns with the slices they meet
            double entries = 0.0;
            for (const ElimDep& d : p.deps[a]) if (!adjoint) entries += 2.0 * n_a * h->integ_dim[d.b];
            for (int b : p.dependents[a]) if (adjoint) entries += 2.0 * n_a * h->integ_dim[b];
            ProfScope ps(h, st, CAT_DYNSOLVE_COUPLE, 8.0 * (double)N * n_cols * (2.0 * n_a + 2.0 * entries));
            launch_elim_couple(st, C, adjoint, store, dB, dY, Bp);
        }
        if (!elim_has_tree(h, a)) {
            ProfScope ps(h, st, CAT_DYNSOLVE_DERIV, 16.0 * (double)N * n_cols * n_a);
            launch_deriv_scan(st, K, n_a, n_cols, D, p.pre[a], adjoint, Bp, dY);
            continue;
        }
        const KRollout R = elim_rollout_args(h, p, a, n_cols);
        dynsolve_load_and_up(h, R, adjoint, h->elim_tree[a].p, Bp, off, S, st);
        dynsolve_descend_all(h, R, adjoint, h->elim_tree[a].p, off, S, Yp, st);
        ProfScope ps(h, st, CAT_DYNSOLVE_SCAN, 0.0);
        launch_elim_collect(st, N, n_a, n_cols, D, p.pre[a], Yp, dY);
    }
}

static void dynamics_solve_all(dto_handle* h, const ElimPlan& p, const double* dZ, int adjoint, const double* dB, int n_cols, double* dY,
                               hipStream_t st) {
    if (h->K < 1) {   // a single knot: the block is the identity
        ProfScope ps(h, st, CAT_DYNSOLVE_SCAN, 0.0);
        HIP_CHECK(hipMemcpyAsync(dY, dB, sizeof(double) * (size_t)n_cols * p.n_states, hipMemcpyDeviceToDevice, st));
        return;
    }
    const ElimWork W = elim_point(h, p, dZ, n_cols, st);
    elim_solve(h, p, W, adjoint, dB, n_cols, dY, st);
}

int dto_dynamics_layout(const dto_handle* h, int32_t* n_states, int32_t* n_levels, int32_t* offset, int32_t* level) {
    if (!h) return fail(nullptr, "null handle");
    dto_handle* hm = const_cast<dto_handle*>(h);   // (the plan is built at the first question and kept)
    try {
        const ElimPlan& p = elim_plan_of(hm);
        if (!p.refusal.empty()) return fail(hm, "dto_dynamics_layout: " + p.refusal);
        if (n_states) *n_states = p.n_states;
        if (n_levels) *n_levels = p.n_levels;
        for (size_t i = 0; i < p.pre.size(); ++i) {
            if (offset) offset[i] = p.pre[i];
            if (level) level[i] = p.level[i];
        }
        return 0;
    } catch (const std::exception& e) {
        return fail(hm, e.what());
    }
}

int dto_dynamics_solve_all(dto_handle* h, const double* Z, int32_t direction, const double* B, int32_t n_cols, double* Y) {
    return guarded(h, [&] {
        const ElimPlan& p = elim_args(h, direction, B, n_cols);
        upload_Z(h, Z);
        const size_t n = (size_t)h->N * n_cols * p.n_states;
        double* dB = grow_workspace(h, h->d_elim_B, n);
        HIP_CHECK(hipMemcpyAsync(dB, B, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
        double* o = staging(h, n);
        dynamics_solve_all(h, p, h->d_Z, direction == DTO_SOLVE_ADJOINT, dB, n_cols, o, h->stream);
        HIP_CHECK(hipMemcpyAsync(Y, o, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_dynamics_solve_all_dev(dto_handle* h, const double* dZ, int32_t direction, const double* dB, int32_t n_cols, double* dY, void* stream) {
    return guarded(h, [&] {
        const ElimPlan& p = elim_args(h, direction, dB, n_cols);
        dynamics_solve_all(h, p, dZ, direction == DTO_SOLVE_ADJOINT, dB, n_cols, dY, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}

// ---- reduced-space operators: the gradient and the Hessian-vector product of the problem with the states eliminated by the dynamics
// (include/dto_engine.h, "Reduced-space operators"; dto_reduced.hip, dto_reduced_plan.h).  Compositions of do_gradient, jac_product,
// dynamics_solve_all (one column) and hess_product, all on `st` and all unchanged; the packers keep every vector on the device.
// With the option "reduced_input_store" the two jac_product calls on the dynamics rows give way to products with the input blocks
// kept beside the coupling blocks (dto_input_plan.h).

// What a reduced-space call names: refused with text before anything is enqueued.
static const ElimPlan& reduced_args(dto_handle* h, const std::string& who, bool hessian) {
    needs_unsharded(h, who);
    const ElimPlan& p = elim_plan_of(h);
    if (!p.refusal.empty()) throw HipError{who + ": " + p.refusal};
    if (h->n_ext_int + h->n_ext_con + h->n_ext_obj > 0)
        throw HipError{who + ": the handle holds host-evaluated terms (" + std::to_string(h->n_ext_int) + " integrators, " +
                       std::to_string(h->n_ext_con) + " constraints, " + std::to_string(h->n_ext_obj) +
                       " objectives): the reduced-space operators run on device-evaluated terms only"};
    if (hessian && !h->eval_hessian) throw HipError{who + ": handle was created with eval_hessian = 0"};
    if (p.n_states < 1) throw HipError{who + ": the handle has no integrator, so no states to eliminate"};
    int64_t rows = 0;
    for (size_t i = 0; i < h->integ_dim.size(); ++i) rows = std::max(rows, h->integ_row_off[i] + h->K * h->integ_dim[i]);
    if (h->n_dyn != h->K * p.n_states || rows > h->n_dyn) throw HipError{who + ": the dynamics rows are not the first (N - 1) n_states rows"};
    return p;
}

// The operators' one block of device memory and the plan's tables, once per handle and before anything is enqueued.
static void reduced_workspaces(dto_handle* h, const ElimPlan& p) {
    if (h->d_red) return;
    std::vector<ReducedIntegrator> its;
    for (size_t i = 0; i < h->integ_kind.size(); ++i)
        its.push_back(ReducedIntegrator{elim_x_off(h, (int)i), h->integ_dim[i], p.pre[i], h->integ_row_off[i]});
    const ReducedPlan rp = reduced_plan(its, h->z);
    const size_t nv = (size_t)h->n_vars, nc = (size_t)std::max<int64_t>(h->n_cons, 1), nd = (size_t)h->N * p.n_states;
    double* blk = dalloc<double>(7 * nv + 4 * nc + 3 * nd);
    int32_t *comp_pos = nullptr, *pos_comp = nullptr, *pos_dim = nullptr, *eq = nullptr;
    int64_t* pos_row = nullptr;
    try {
        comp_pos = dupload(rp.comp_pos); pos_comp = dupload(rp.pos_comp); pos_dim = dupload(rp.pos_dim); pos_row = dupload(rp.pos_row);
        eq = dalloc<int32_t>(1);
    } catch (...) {
        for (void* q : {(void*)blk, (void*)comp_pos, (void*)pos_comp, (void*)pos_dim, (void*)pos_row}) if (q) (void)hipFree(q);
        throw;
    }
    h->red = KReduced{own(h, comp_pos), own(h, pos_comp), own(h, pos_dim), own(h, pos_row), h->z, p.n_states, h->N, h->n_vars, h->n_cons, h->n_dyn};
    h->red_point.d_flag = own(h, eq);
    double* q = blk;
    auto take = [&](size_t n) { double* r = q; q += n; return r; };
    h->red_point.d_Z = take(nv); h->red_g = take(nv); h->red_r = take(nv); h->red_a = take(nv); h->red_b = take(nv); h->red_hv = take(nv); h->red_out = take(nv);
    h->red_point.d_mu = take(nc); h->red_mut = take(nc); h->red_w = take(nc); h->red_hmu = take(nc);
    h->red_lam = take(nd); h->red_s1 = take(nd); h->red_s2 = take(nd);
    h->d_red = own(h, blk);
}

// bytes of the two products with the input blocks (h->input exists: the solves' point was ensured with the option on): the store once,
// the free inputs of v and B, or q, Gam and y
static double input_forward_bytes(const dto_handle* h) {
    return 8.0 * ((double)h->input->store_off.back() + (double)h->N * (h->in.n_read + 2.0 * h->red.D));
}
static double input_transposed_bytes(const dto_handle* h) {
    return 8.0 * ((double)h->input->store_off.back() + 2.0 * (double)h->n_vars + (double)h->N * h->red.D);
}

// The reduced point: g, Lam, mu~ and the reduced gradient at (Z, sigma, mu or "mu = NULL"), computed unless red_point keeps them.
static void reduced_point(dto_handle* h, const ElimPlan& p, const double* dZ, double sigma, const double* dmu, hipStream_t st) {
    const KReduced& R = h->red;
    const double nv = 8.0 * (double)h->n_vars, nc = 8.0 * (double)h->n_cons, nd = 8.0 * (double)h->N * R.D;
    if (at_kept_point(h, h->red_point, st, dZ, sigma, dmu)) return;
    do_gradient(h, dZ, h->red_a, st);
    const double* t1 = nullptr;
    if (dmu) {   // J' w1, w1 = mu with its dynamics rows zeroed
        { ProfScope ps(h, st, CAT_REDUCED_PACK, 2.0 * nc); launch_red_multipliers(st, R, nullptr, dmu, 1, h->red_w, nullptr); }
        jac_product(h, dZ, h->red_w, h->red_b, 1, st);
        t1 = h->red_b;
    }
    { ProfScope ps(h, st, CAT_REDUCED_PACK, (t1 ? 3.0 : 2.0) * nv + nd); launch_red_gradient(st, R, sigma, h->red_a, t1, h->red_g, h->red_s1); }
    dynamics_solve_all(h, p, dZ, 1, h->red_s1, 1, h->red_lam, st);
    { ProfScope ps(h, st, CAT_REDUCED_PACK, nd + (dmu ? 3.0 : 2.0) * nc); launch_red_multipliers(st, R, h->red_lam, dmu, 0, h->red_w, h->red_mut); }
    if (h->reduced_input_store && h->K >= 1) {   // t = J' w2 from the input blocks the adjoint solve's point holds
        ProfScope ps(h, st, CAT_REDUCED_INPUT, input_transposed_bytes(h));
        launch_red_input_transposed(st, R, h->in, h->d_in_store.p, h->red_g, h->red_lam, h->red_r);
    } else {
        jac_product(h, dZ, h->red_w, h->red_b, 1, st);
        { ProfScope ps(h, st, CAT_REDUCED_PACK, 3.0 * nv); launch_red_finish(st, R, h->red_g, h->red_b, h->red_lam, h->red_r); }
    }
    keep_point(h, h->red_point, st, dZ, sigma, dmu);
}

// The device routines both entry-point families run: everything on `st`, every pointer a device pointer.
static void reduced_gradient(dto_handle* h, const ElimPlan& p, const double* dZ, double sigma, const double* dmu, double* dgrad, double* dlam,
                             hipStream_t st) {
    reduced_point(h, p, dZ, sigma, dmu, st);
    if (dgrad) HIP_CHECK(hipMemcpyAsync(dgrad, h->red_r, sizeof(double) * (size_t)h->n_vars, hipMemcpyDeviceToDevice, st));
    if (dlam) HIP_CHECK(hipMemcpyAsync(dlam, h->red_lam, sizeof(double) * (size_t)h->N * h->red.D, hipMemcpyDeviceToDevice, st));
}

// y = T' H(Z; sigma, mu~) T v.  At the reduced point's (Z, sigma, mu): steps 1 .. 8 of the header alone.
static void reduced_hessian_product(dto_handle* h, const ElimPlan& p, const double* dZ, double sigma, const double* dmu, const double* dv,
                                    double* dy, hipStream_t st) {
    reduced_point(h, p, dZ, sigma, dmu, st);
    const KReduced& R = h->red;
    const double nv = 8.0 * (double)h->n_vars, nc = 8.0 * (double)h->n_cons, nd = 8.0 * (double)h->N * R.D;
    if (h->reduced_input_store && h->K >= 1) {
        // The reduced point and the solves' point are kept apart: a dto_dynamics_solve_all at another Z in between leaves the first
        // valid and the input blocks stale.  So the solves' point is made this Z BEFORE the first kernel reads the store (one compare;
        // after such a call one rebuild with one Jacobian evaluation), and both solves then run at it without a compare of their own.
        const ElimWork W = elim_point(h, p, dZ, 1, st);
        { ProfScope ps(h, st, CAT_REDUCED_INPUT, input_forward_bytes(h)); launch_red_input_forward(st, R, h->in, h->d_in_store.p, dv, h->red_s1); }
        elim_solve(h, p, W, 0, h->red_s1, 1, h->red_s2, st);                    // MM Y = B
        { ProfScope ps(h, st, CAT_REDUCED_PACK, 2.0 * nv); launch_red_zhat(st, R, dv, h->red_s2, h->red_a); }
        hess_product(h, dZ, sigma, h->red_mut, h->red_a, h->red_b, st);         // q = H(mu~) z^
        { ProfScope ps(h, st, CAT_REDUCED_PACK, 2.0 * nd); launch_red_gather(st, R, h->red_b, h->red_s1); }
        elim_solve(h, p, W, 1, h->red_s1, 1, h->red_s2, st);                    // MM' Gam = q_S
        ProfScope ps(h, st, CAT_REDUCED_INPUT, input_transposed_bytes(h));
        launch_red_input_transposed(st, R, h->in, h->d_in_store.p, h->red_b, h->red_s2, dy);
        return;
    }
    { ProfScope ps(h, st, CAT_REDUCED_PACK, 2.0 * nv); launch_red_vhat(st, R, dv, h->red_a); }
    jac_product(h, dZ, h->red_a, h->red_w, 0, st);                          // rho = J v^
    { ProfScope ps(h, st, CAT_REDUCED_PACK, 2.0 * nd); launch_red_rhs(st, R, dv, h->red_w, h->red_s1); }
    dynamics_solve_all(h, p, dZ, 0, h->red_s1, 1, h->red_s2, st);           // MM Y = B
    { ProfScope ps(h, st, CAT_REDUCED_PACK, 2.0 * nv); launch_red_zhat(st, R, dv, h->red_s2, h->red_a); }
    hess_product(h, dZ, sigma, h->red_mut, h->red_a, h->red_b, st);         // q = H(mu~) z^
    { ProfScope ps(h, st, CAT_REDUCED_PACK, 2.0 * nd); launch_red_gather(st, R, h->red_b, h->red_s1); }
    dynamics_solve_all(h, p, dZ, 1, h->red_s1, 1, h->red_s2, st);           // MM' Gam = q_S
    { ProfScope ps(h, st, CAT_REDUCED_PACK, nd + nc); launch_red_multipliers(st, R, h->red_s2, nullptr, 0, h->red_w, nullptr); }
    jac_product(h, dZ, h->red_w, h->red_a, 1, st);                          // t = J' w
    { ProfScope ps(h, st, CAT_REDUCED_PACK, 3.0 * nv); launch_red_finish(st, R, h->red_b, h->red_a, h->red_s2, dy); }
}

int dto_reduced_gradient(dto_handle* h, const double* Z, double sigma, const double* mu, double* grad, double* lam) {
    return guarded(h, [&] {
        const std::string who = "dto_reduced_gradient";
        const ElimPlan& p = reduced_args(h, who, false);
        if (!Z || !grad) throw HipError{who + ": Z and grad are required (NULL given)"};
        reduced_workspaces(h, p);
        upload_Z(h, Z);
        if (mu && h->n_cons > 0) HIP_CHECK(hipMemcpyAsync(h->red_hmu, mu, sizeof(double) * (size_t)h->n_cons, hipMemcpyHostToDevice, h->stream));
        reduced_point(h, p, h->d_Z, sigma, mu ? h->red_hmu : nullptr, h->stream);
        HIP_CHECK(hipMemcpyAsync(grad, h->red_r, sizeof(double) * (size_t)h->n_vars, hipMemcpyDeviceToHost, h->stream));
        if (lam) HIP_CHECK(hipMemcpyAsync(lam, h->red_lam, sizeof(double) * (size_t)h->N * p.n_states, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_reduced_gradient_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, double* dgrad, double* dlam, void* stream) {
    return guarded(h, [&] {
        const std::string who = "dto_reduced_gradient_dev";
        const ElimPlan& p = reduced_args(h, who, false);
        if (!dZ || !dgrad) throw HipError{who + ": dZ and dgrad are required (NULL given)"};
        reduced_workspaces(h, p);
        reduced_gradient(h, p, dZ, sigma, dmu, dgrad, dlam, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}
int dto_reduced_hessian_product(dto_handle* h, const double* Z, double sigma, const double* mu, const double* v, double* y) {
    return guarded(h, [&] {
        const std::string who = "dto_reduced_hessian_product";
        const ElimPlan& p = reduced_args(h, who, true);
        if (!Z || !v || !y) throw HipError{who + ": Z, v and y are required (NULL given)"};
        reduced_workspaces(h, p);
        upload_Z(h, Z);
        if (mu && h->n_cons > 0) HIP_CHECK(hipMemcpyAsync(h->red_hmu, mu, sizeof(double) * (size_t)h->n_cons, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(h->red_hv, v, sizeof(double) * (size_t)h->n_vars, hipMemcpyHostToDevice, h->stream));
        reduced_hessian_product(h, p, h->d_Z, sigma, mu ? h->red_hmu : nullptr, h->red_hv, h->red_out, h->stream);
        HIP_CHECK(hipMemcpyAsync(y, h->red_out, sizeof(double) * (size_t)h->n_vars, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_reduced_hessian_product_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* dv, double* dy, void* stream) {
    return guarded(h, [&] {
        const std::string who = "dto_reduced_hessian_product_dev";
        const ElimPlan& p = reduced_args(h, who, true);
        if (!dZ || !dv || !dy) throw HipError{who + ": dZ, dv and dy are required (NULL given)"};
        reduced_workspaces(h, p);
        reduced_hessian_product(h, p, dZ, sigma, dmu, dv, dy, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}

// ---- block products: H V and T' H T V for n_cols vectors per call (include/dto_engine.h, "Block products").  Per column the
// operations of the single products in their order, so the same bits; what a block saves is the re-reading of the matrices: the
// Hessian copy once per tile of columns, the solves' node matrices and the input blocks once per chunk.

static const int BLOCK_WIDTH_DEFAULT = 64;   // W_max (DESIGN 4.29 holds the table it was chosen from)

static int block_width(const dto_handle* h, int cap) {
    const int width = h->reduced_block_width > 0 ? h->reduced_block_width : BLOCK_WIDTH_DEFAULT;
    return std::max(1, std::min(cap, width));
}

static void block_args(const std::string& who, int32_t n_cols, const double* Z, const double* V, double* Y) {
    if (n_cols < 1) throw HipError{who + ": n_cols = " + std::to_string(n_cols) + ", at least 1 column is required"};
    if (!Z || !V || !Y) throw HipError{who + ": Z, V and Y are required (NULL given)"};
}

// Y = H(Z; sigma, mu) V, V and Y [n_cols][n_vars] on the device: one point check, then one launch per chunk of W columns.
static void hess_products(dto_handle* h, const double* dZ, double sigma, const double* dmu, int n_cols, const double* dV, double* dY,
                          hipStream_t st) {
    const int W = block_width(h, 64);
    const int64_t nv = h->n_vars;
    hess_point(h, dZ, sigma, dmu, st);
    for (int c0 = 0; c0 < n_cols; c0 += W) {
        const int w = std::min(W, n_cols - c0);
        hess_product_block(h, KHessBlock{w, 1, nv, 1, nv}, dV + (size_t)c0 * nv, dY + (size_t)c0 * nv, st);
    }
}

// the host-pointer forms' copies of V and Y, [n_cols][n_vars] each
static double* block_host_buffers(dto_handle* h, int n_cols) { return grow_workspace(h, h->d_blk_host, 2 * (size_t)n_cols * (size_t)h->n_vars); }

int dto_eval_hessian_products(dto_handle* h, const double* Z, double sigma, const double* mu, int32_t n_cols, const double* V, double* Y) {
    return guarded(h, [&] {
        hess_product_applies(h);
        block_args("dto_eval_hessian_products", n_cols, Z, V, Y);
        if (!mu && h->n_cons > 0) throw HipError{"dto_eval_hessian_products: mu = NULL (the multipliers [n_cons] are required)"};
        const size_t n = (size_t)n_cols * (size_t)h->n_vars;
        double* dV = block_host_buffers(h, n_cols);
        upload_Z(h, Z);
        if (h->n_cons > 0) HIP_CHECK(hipMemcpyAsync(h->d_mu, mu, sizeof(double) * (size_t)h->n_cons, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(dV, V, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
        hess_products(h, h->d_Z, sigma, h->d_mu, n_cols, dV, dV + n, h->stream);
        HIP_CHECK(hipMemcpyAsync(Y, dV + n, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_eval_hessian_products_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, int32_t n_cols, const double* dV, double* dY,
                                  void* stream) {
    return guarded(h, [&] {
        hess_product_applies(h);
        block_args("dto_eval_hessian_products_dev", n_cols, dZ, dV, dY);
        hess_products(h, dZ, sigma, dmu, n_cols, dV, dY, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}

// ---- augmented-Lagrangian terms (include/dto_engine.h, "Augmented-Lagrangian terms"; dto_auglag.hip, dto_auglag_plan.h): the row pass
// and the Gauss-Newton term the reduced-space calls below take in.

// d_al's vectors: mu_eff, weight, g, the single-column route's rows and the host-pointer forms' mu and rho [n_cons] each, info [8]
struct AlWork { double *mu_eff, *weight, *g, *rows, *hmu, *hrho, *info; };

// Every workspace of the terms, before anything is enqueued: d_al (once per handle), the planes t for chunks of W columns (W = 0: a call
// without products) and the rows' equality flags.
static AlWork auglag_workspaces(dto_handle* h, int W) {
    const size_t nc = (size_t)std::max<int64_t>(h->n_cons, 1);
    double* q = grow_workspace(h, h->d_al, 6 * nc + AL_INFO);
    if (W > 0) grow_workspace(h, h->d_al_t, (size_t)W * (size_t)h->n_vars);
    if (!h->d_al_eq) {
        std::vector<unsigned char> eq((size_t)std::max<int64_t>(h->n_cons - h->n_dyn, 1), 0);
        for (auto& c : h->con)
            for (int64_t i = 0; i < c.n_times_total * c.g_dim; ++i) eq[(size_t)(c.row_off - h->n_dyn + i)] = c.equality ? 1 : 0;
        h->d_al_eq = own(h, dupload(eq));
    }
    return AlWork{q, q + nc, q + 2 * nc, q + 3 * nc, q + 4 * nc, q + 5 * nc, q + 6 * nc};
}

// The row pass at g (the non-dynamics rows are read): mu_eff / weight / info where given; with dphi, phi = sigma * f + P.
static void auglag_row_pass(dto_handle* h, const double* g, const double* dmu, const double* drho, double* mu_eff, double* weight, double* info,
                            double sigma, const double* f, double* dphi, hipStream_t st) {
    const double rows = (double)(h->n_cons - h->n_dyn), outs = (mu_eff ? 8.0 : 0.0) + (weight ? 8.0 : 0.0);
    ProfScope ps(h, st, CAT_AUGLAG, rows * (17.0 + (dmu ? 8.0 : 0.0) + outs) + outs * (double)h->n_dyn + 8.0 * AL_INFO + (dphi ? 16.0 : 0.0));
    launch_al_rows(st, KAlRows{h->n_dyn, h->n_cons, h->d_al_eq, g, dmu, drho, mu_eff, weight, info, sigma, f, dphi});
}

// The row pass at Z into the handle's mu_eff and weight: the non-dynamics rows of g from the constraints' value launchers alone -- no
// sweep, no chain.
static void auglag_rows_at(dto_handle* h, const AlWork& A, const double* dZ, const double* dmu, const double* drho, double* info, hipStream_t st) {
    for (auto& c : h->con) launch_cons_knot(st, h->P, c.k, dZ, A.g);
    auglag_row_pass(h, A.g, dmu, drho, A.mu_eff, A.weight, info, 0.0, nullptr, nullptr, st);
}

// q_j <- q_j + t_j, t_j = J_c' (W (J_c z^_j)), for the w columns of a chunk; z^ and q planes [w][n_vars].  t is formed from zeros by the
// constraints in list order: a constraint ||v|| - c or ||v||^2 - c that repeats neither a knot nor a component in ONE launch for all
// columns, any other (the quadratic form, a repeated knot or component) through the products' own single-column launchers around the
// scaling.  Then the one rounded addition.
static void auglag_gauss_newton(dto_handle* h, const AlWork& A, const double* dZ, int w, const double* zh, double* q, hipStream_t st) {
    const int64_t nv = h->n_vars;
    const size_t n = (size_t)w * (size_t)nv;
    double* t = h->d_al_t.p;
    if (!jac_product_is_matrix_free(h, 0) || !jac_product_is_matrix_free(h, 1)) {
        // A handle whose public products take the value-slab route (jac_product_is_matrix_free: time-dependent integrators without
        // "tdb_matrix_free_products", ..) sums a row across lanes, not in k_jv_knot's order.  There the term IS the two public
        // products around the scaling, one column at a time -- what the same handle's projected_chunk does for J v^ and J' w off
        // the store route.
        const int64_t rows = h->n_cons - h->n_dyn;
        for (int j = 0; j < w; ++j) {
            jac_product(h, dZ, zh + (size_t)j * nv, A.rows, 0, st);
            HIP_CHECK(hipMemsetAsync(A.rows, 0, sizeof(double) * (size_t)h->n_dyn, st));
            { ProfScope ps(h, st, CAT_AUGLAG, 24.0 * (double)rows); launch_al_scale(st, rows, A.weight + h->n_dyn, A.rows + h->n_dyn); }
            jac_product(h, dZ, A.rows, t + (size_t)j * nv, 1, st);
        }
        ProfScope ps(h, st, CAT_AUGLAG, 24.0 * (double)n);
        launch_al_add(st, (int64_t)n, t, q);
        return;
    }
    HIP_CHECK(hipMemsetAsync(t, 0, sizeof(double) * n, st));
    for (auto& c : h->con) {
        const KCon& k = c.k;
        if (k.n_times <= 0) continue;
        if ((k.kind == DTO_CONSTRAINT_NORM_MINUS_C || k.kind == DTO_CONSTRAINT_SQNORM_MINUS_C) && !k.repeats && !k.comp_repeats) {
            // per thread: the listing's components of Z and z^ with their pattern flags, the row's weight, its entry of t twice
            ProfScope ps(h, st, CAT_AUGLAG, 8.0 * (double)k.n_times * k.n_comps * w * (3.0 * k.n_comps + 3.0));
            launch_al_gn(st, h->P, k, w, nv, dZ, A.weight, zh, t);
            continue;
        }
        const int64_t rows = c.n_times_total * c.g_dim;
        for (int j = 0; j < w; ++j) {
            HIP_CHECK(hipMemsetAsync(A.rows + c.row_off, 0, sizeof(double) * (size_t)rows, st));
            launch_jv_knot(st, h->P, k, dZ, zh + (size_t)j * nv, A.rows, 0);
            { ProfScope ps(h, st, CAT_AUGLAG, 24.0 * (double)rows); launch_al_scale(st, rows, A.weight + c.row_off, A.rows + c.row_off); }
            launch_jv_knot(st, h->P, k, dZ, A.rows, t + (size_t)j * nv, 1);
        }
    }
    ProfScope ps(h, st, CAT_AUGLAG, 24.0 * (double)n);
    launch_al_add(st, (int64_t)n, t, q);
}

// one chunk's vectors inside d_blk
struct BlockWork { double *s1, *s2, *zh, *q, *rows; };

// Every workspace of a projected block call, before anything is enqueued: d_blk for chunks of W columns (rows only off the store route)
// and, through elim_point below, what the solves grow for n_cols = W.
static BlockWork block_workspaces(dto_handle* h, const ElimPlan& p, int W, bool store_route) {
    const size_t nv = (size_t)h->n_vars, nc = (size_t)std::max<int64_t>(h->n_cons, 1), nd = (size_t)h->N * p.n_states;
    double* q = grow_workspace(h, h->d_blk, (size_t)W * (2 * nd + 2 * nv + (store_route ? 0 : nc)));
    BlockWork B{};
    B.s1 = q; q += W * nd;
    B.s2 = q; q += W * nd;
    B.zh = q; q += W * nv;
    B.q = q; q += W * nv;
    B.rows = store_route ? nullptr : q;
    return B;
}

// columns per chunk of a projected block call: W = min(the solves' limit, the option or W_max), and no more than the call has
static int projected_width(const dto_handle* h, int n_cols) { return std::min(block_width(h, elim_column_cap(h)), n_cols); }

// The three points a projected product works at -- the reduced point, the solves' point (workspaces for W columns) and the Hessian
// point at mu~ -- each checked once: at a new Z the rebuild the single product would run at its first solve (on the store route:
// before its first kernel) runs here.
static ElimWork projected_points(dto_handle* h, const ElimPlan& p, const double* dZ, double sigma, const double* dmu, int W, hipStream_t st) {
    ElimWork EW{};
    reduced_point(h, p, dZ, sigma, dmu, st);
    if (h->K >= 1) EW = elim_point(h, p, dZ, W, st);
    hess_point(h, dZ, sigma, h->red_mut, st);
    return EW;
}

// One chunk of w columns at the points projected_points ensured: y = T' H(Z; sigma, mu~) T v, v and y [w][n_vars], in B's vectors --
// the steps of reduced_hessian_product in block form.  With `al` (the dto_auglag_* calls with penalties) the Gauss-Newton term
// J_c' W J_c z^ joins q behind the Hessian product; without it the launches are the ones they were.
static void projected_chunk(dto_handle* h, const ElimPlan& p, const BlockWork& B, const ElimWork& EW, bool store_route, const double* dZ,
                            int w, const double* v, double* y, hipStream_t st, const AlWork* al = nullptr) {
    const KReduced& R = h->red;
    const int64_t nvars = h->n_vars, ncons = h->n_cons;
    auto solve = [&](int adjoint, int w) {
        if (h->K < 1) {   // a single knot: the block is the identity
            ProfScope ps(h, st, CAT_DYNSOLVE_SCAN, 0.0);
            HIP_CHECK(hipMemcpyAsync(B.s2, B.s1, sizeof(double) * (size_t)w * p.n_states, hipMemcpyDeviceToDevice, st));
            return;
        }
        elim_solve(h, p, EW, adjoint, B.s1, w, B.s2, st);
    };
    {
        const double nv = 8.0 * (double)nvars * w, nc = 8.0 * (double)ncons * w, nd = 8.0 * (double)h->N * R.D * w;
        const KHessBlock HB{w, 1, nvars, 1, nvars};   // z^ and q as planes [w][n_vars], like V and Y (faster than interleaved)
        if (store_route) {
            {   // bytes: the store once, per column the free inputs of v and B
                ProfScope ps(h, st, CAT_REDUCED_INPUT, 8.0 * (double)h->input->store_off.back() + 8.0 * (double)h->N * w * (h->in.n_read + 2.0 * R.D));
                launch_red_input_forward_block(st, R, h->in, w, h->d_in_store.p, v, B.s1);
            }
            solve(0, w);                                                                                   // MM Y = B
            { ProfScope ps(h, st, CAT_REDUCED_PACK, 2.0 * nv); launch_red_zhat_block(st, R, w, v, B.s2, B.zh); }
            hess_product_block(h, HB, B.zh, B.q, st);                                                      // q = H(mu~) z^
            if (al) auglag_gauss_newton(h, *al, dZ, w, B.zh, B.q, st);                                     // q += J_c' W J_c z^
            { ProfScope ps(h, st, CAT_REDUCED_PACK, 2.0 * nd); launch_red_gather_block(st, R, w, B.q, B.s1); }
            solve(1, w);                                                                                   // MM' Gam = q_S
            // bytes: the store once, per column q, Gam and y
            ProfScope ps(h, st, CAT_REDUCED_INPUT, 8.0 * (double)h->input->store_off.back() + 2.0 * nv + nd);
            launch_red_input_transposed_block(st, R, h->in, w, h->d_in_store.p, B.q, B.s2, y);
            return;
        }
        // z^'s buffer holds v^ and later t, rows holds rho and later w: planes, since J v^ and J' w take one column at a time
        { ProfScope ps(h, st, CAT_REDUCED_PACK, 2.0 * nv); launch_red_vhat_block(st, R, w, v, B.zh); }
        for (int j = 0; j < w; ++j) jac_product(h, dZ, B.zh + (size_t)j * nvars, B.rows + (size_t)j * ncons, 0, st);   // rho = J v^
        { ProfScope ps(h, st, CAT_REDUCED_PACK, 2.0 * nd); launch_red_rhs_block(st, R, w, v, B.rows, B.s1); }
        solve(0, w);                                                                                       // MM Y = B
        { ProfScope ps(h, st, CAT_REDUCED_PACK, 2.0 * nv); launch_red_zhat_block(st, R, w, v, B.s2, B.zh); }
        hess_product_block(h, HB, B.zh, B.q, st);                                                          // q = H(mu~) z^
        if (al) auglag_gauss_newton(h, *al, dZ, w, B.zh, B.q, st);                                         // q += J_c' W J_c z^
        { ProfScope ps(h, st, CAT_REDUCED_PACK, 2.0 * nd); launch_red_gather_block(st, R, w, B.q, B.s1); }
        solve(1, w);                                                                                       // MM' Gam = q_S
        { ProfScope ps(h, st, CAT_REDUCED_PACK, nd + nc); launch_red_multipliers_block(st, R, w, B.s2, B.rows); }
        for (int j = 0; j < w; ++j) jac_product(h, dZ, B.rows + (size_t)j * ncons, B.zh + (size_t)j * nvars, 1, st);   // t = J' w
        { ProfScope ps(h, st, CAT_REDUCED_PACK, 3.0 * nv); launch_red_finish_block(st, R, w, B.q, B.zh, B.s2, y); }
    }
}

// Y = T' H(Z; sigma, mu~) T V, V and Y [n_cols][n_vars] on the device.  The three point checks (reduced point, solves' point, Hessian
// point) once; then per chunk of w <= W columns the steps of reduced_hessian_product in block form.
static void projected_hessian_products(dto_handle* h, const ElimPlan& p, const double* dZ, double sigma, const double* dmu, int n_cols,
                                       const double* dV, double* dY, hipStream_t st, const AlWork* al = nullptr) {
    const int W = projected_width(h, n_cols);
    const bool store_route = h->reduced_input_store && h->K >= 1;
    // the block's and (in projected_points) the solves' workspaces for W columns first: a failed allocation is refused before anything
    // is enqueued
    const BlockWork B = block_workspaces(h, p, W, store_route);
    const ElimWork EW = projected_points(h, p, dZ, sigma, dmu, W, st);
    for (int c0 = 0; c0 < n_cols; c0 += W)
        projected_chunk(h, p, B, EW, store_route, dZ, std::min(W, n_cols - c0), dV + (size_t)c0 * h->n_vars, dY + (size_t)c0 * h->n_vars, st, al);
}

// ---- truncated-Newton step: Steihaug-Toint CG on A = M (T'HT) M + shift M (include/dto_engine.h, "Truncated-Newton step"; dto_newton.hip,
// dto_newton_plan.h).  The product of an iteration is the one-column chunk of the block products above -- the single product's bits --
// at points checked once per call; the dots, the updates and the decisions are four small kernels, and what the host reads per
// iteration is (status, iterations) through the mailbox.

// What a step names: refused with text before the handle is touched, so a structure-only handle answers these too.
static std::string newton_refusal(const std::string& who, const double* Z, double radius, double shift, double rtol, double atol, int32_t max_iter,
                                  const double* p, const double* info) {
    if (!Z || !p || !info) return who + ": Z, p and info are required (NULL given)";
    if (max_iter < 1) return who + ": max_iter = " + std::to_string(max_iter) + ", at least 1 iteration is required";
    if (!std::isfinite(radius) || radius < 0.0) return who + ": radius must be finite and >= 0 (0: no trust region)";
    if (!std::isfinite(rtol) || rtol < 0.0) return who + ": rtol must be finite and >= 0";
    if (!std::isfinite(atol) || atol < 0.0) return who + ": atol must be finite and >= 0";
    if (!std::isfinite(shift)) return who + ": shift must be finite";
    return "";
}

// The device routine both entry-point families run: everything on `st`, every pointer a device pointer (dmu, dmask, dtrace may be null).
static void newton_step(dto_handle* h, const ElimPlan& p, const double* dZ, double sigma, const double* dmu, const double* dmask, double radius,
                        double shift, double rtol, double atol, int max_iter, double* dp, double* dinfo, double* dtrace, hipStream_t st) {
    const KReduced& R = h->red;
    const int64_t n = h->n_vars, nb = newton_chunks(n);
    const bool store_route = h->reduced_input_store && h->K >= 1;
    // every workspace before anything is enqueued
    double* q = grow_workspace(h, h->d_newton, (size_t)newton_workspace_doubles(n));
    const BlockWork B = block_workspaces(h, p, 1, store_route);
    KNewton A{};
    A.n = n; A.nb = nb;
    A.p = dp; A.r = q; A.d = q + n; A.w = q + 2 * n;
    A.part = q + 3 * n; A.state = A.part + NEWTON_SLOTS * nb;
    A.g = h->red_r; A.mask = dmask; A.info = dinfo; A.trace = dtrace;
    A.radius = radius; A.shift = shift; A.rtol = rtol; A.atol = atol;
    static const int combine_launch = tune_int("DTO_NEWTON_COMBINE", 0);   // A/B runs (TUNING builds): 1 = stage 2 of the dots in a launch of its own
    A.combined = combine_launch ? 1 : 0;
    auto combine = [&](int slot0, int count) {
        if (!A.combined) return;
        ProfScope ps(h, st, CAT_NEWTON, 8.0 * (double)nb * count);
        launch_newton_combine(st, A, slot0, count);
    };
    const ElimWork EW = projected_points(h, p, dZ, sigma, dmu, 1, st);
    // bytes as executed: the vectors each kernel reads and writes (the mask where one is given), its partial sums, and per workgroup
    // the partial sums it combines
    const double v = 8.0 * (double)n, m = dmask ? v : 0.0, part = 8.0 * (double)nb, groups = (double)((nb + 15) / 16);
    auto running = [&] {   // the one readback per iteration
        HIP_CHECK(hipMemcpyAsync(h->mailbox->newton, A.state, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return (int)h->mailbox->newton[NWS_STATUS] == NEWTON_CONTINUE;
    };
    { ProfScope ps(h, st, CAT_NEWTON, 4.0 * v + m + part); launch_newton_start(st, R, A); }
    combine(NWT_RR, 1);
    { ProfScope ps(h, st, CAT_NEWTON, groups * part); launch_newton_dir(st, A, 0, max_iter); }
    for (int j = 1; j <= max_iter && running(); ++j) {
        projected_chunk(h, p, B, EW, store_route, dZ, 1, A.d, A.w, st);   // y = T'HT d
        { ProfScope ps(h, st, CAT_NEWTON, 4.0 * v + m + 4.0 * part); launch_newton_curv(st, R, A); }
        combine(NWT_KAPPA, 4);
        { ProfScope ps(h, st, CAT_NEWTON, 7.0 * v + m + 4.0 * part + groups * 4.0 * part); launch_newton_step(st, R, A, j); }
        combine(NWT_RR, 4);
        { ProfScope ps(h, st, CAT_NEWTON, 3.0 * v + (groups + 3.0) * part); launch_newton_dir(st, A, j, max_iter); }
    }
}

int dto_projected_newton_step(dto_handle* h, const double* Z, double sigma, const double* mu, const double* free_mask, double radius,
                              double shift, double rtol, double atol, int32_t max_iter, double* p, double* info, double* trace) {
    const std::string who = "dto_projected_newton_step";
    if (!h) return fail(nullptr, "null handle");
    const std::string bad = newton_refusal(who, Z, radius, shift, rtol, atol, max_iter, p, info);
    if (!bad.empty()) return fail(h, bad);
    return guarded(h, [&] {
        const ElimPlan& ep = reduced_args(h, who, true);
        reduced_workspaces(h, ep);
        const size_t n = (size_t)h->n_vars, nt = 4 * (size_t)max_iter;
        grow_workspace(h, h->d_newton, (size_t)newton_workspace_doubles(h->n_vars));   // before the uploads are enqueued
        block_workspaces(h, ep, 1, h->reduced_input_store && h->K >= 1);
        double* q = grow_workspace(h, h->d_newton_host, 2 * n + 8 + nt);
        double *dmask = q, *dp = q + n, *dinfo = q + 2 * n, *dtrace = dinfo + 8;
        upload_Z(h, Z);
        if (mu && h->n_cons > 0) HIP_CHECK(hipMemcpyAsync(h->red_hmu, mu, sizeof(double) * (size_t)h->n_cons, hipMemcpyHostToDevice, h->stream));
        if (free_mask) HIP_CHECK(hipMemcpyAsync(dmask, free_mask, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
        // the rows of the trace the step does not reach keep the caller's values
        if (trace) HIP_CHECK(hipMemcpyAsync(dtrace, trace, sizeof(double) * nt, hipMemcpyHostToDevice, h->stream));
        newton_step(h, ep, h->d_Z, sigma, mu ? h->red_hmu : nullptr, free_mask ? dmask : nullptr, radius, shift, rtol, atol, max_iter, dp, dinfo,
                    trace ? dtrace : nullptr, h->stream);
        HIP_CHECK(hipMemcpyAsync(p, dp, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipMemcpyAsync(info, dinfo, sizeof(double) * 8, hipMemcpyDeviceToHost, h->stream));
        if (trace) HIP_CHECK(hipMemcpyAsync(trace, dtrace, sizeof(double) * nt, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_projected_newton_step_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* dfree_mask, double radius,
                                  double shift, double rtol, double atol, int32_t max_iter, double* dp, double* dinfo, double* dtrace, void* stream) {
    const std::string who = "dto_projected_newton_step_dev";
    if (!h) return fail(nullptr, "null handle");
    const std::string bad = newton_refusal(who, dZ, radius, shift, rtol, atol, max_iter, dp, dinfo);
    if (!bad.empty()) return fail(h, bad);
    return guarded(h, [&] {
        const ElimPlan& ep = reduced_args(h, who, true);
        reduced_workspaces(h, ep);
        newton_step(h, ep, dZ, sigma, dmu, dfree_mask, radius, shift, rtol, atol, max_iter, dp, dinfo, dtrace, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}

// ---- bound-constrained truncated-Newton step (include/dto_engine.h, "Bound-constrained truncated-Newton step"; dto_newton_box.hip,
// dto_newton_box_plan.h): newton_step's shape with lower and upper bounds on the independent entries.

// [a, a + n) and [b, b + n) share an entry (a null pointer overlaps nothing)
static bool ranges_overlap(const double* a, const double* b, size_t n) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = n * sizeof(double);
    return x < y + len && y < x + len;
}

// What a box step names beyond newton_refusal: the outputs must not overlap Z, the mask or the bounds.
static std::string newton_box_refusal(const std::string& who, size_t n, const double* Z, const double* mask, const double* lo, const double* hi,
                                      const double* p, const double* zp, const double* es) {
    const std::pair<const char*, const double*> outs[] = {{"p", p}, {"Zp", zp}, {"entry_state", es}};
    const std::pair<const char*, const double*> ins[] = {{"Z", Z}, {"free_mask", mask}, {"lo", lo}, {"hi", hi}};
    for (const auto& o : outs)
        for (const auto& i : ins)
            if (ranges_overlap(o.second, i.second, n)) return who + ": " + o.first + " overlaps " + i.first;
    return "";
}

struct NewtonBoxArgs {
    const double *mask, *lo, *hi;       // device pointers or null
    double radius, shift, rtol, atol;
    int max_iter;
    double *p, *info, *trace, *entry_state, *zp;
};

// The device routine both entry-point families run: everything on `st`, every pointer a device pointer.
static void newton_box_step(dto_handle* h, const ElimPlan& p, const double* dZ, double sigma, const double* dmu, const NewtonBoxArgs& a, hipStream_t st,
                            const AlWork* al = nullptr) {
    const KReduced& R = h->red;
    const int64_t n = h->n_vars, nb = newton_chunks(n);
    const bool store_route = h->reduced_input_store && h->K >= 1;
    // every workspace before anything is enqueued
    double* q = grow_workspace(h, h->d_newton_box, (size_t)newton_box_workspace_doubles(n));
    const BlockWork B = block_workspaces(h, p, 1, store_route);
    KNewtonBox A{};
    A.n = n; A.nb = nb;
    A.p = a.p; A.r = q; A.d = q + n; A.w = q + 2 * n;
    A.part = q + 3 * n; A.state = A.part + NEWTON_BOX_SLOTS * nb;
    A.es = (unsigned char*)(A.state + NEWTON_BOX_STATE);
    A.g = h->red_r; A.mask = a.mask; A.Z = dZ; A.lo = a.lo; A.hi = a.hi;
    A.info = a.info; A.trace = a.trace; A.zp = a.zp; A.es_out = a.entry_state;
    A.radius = a.radius; A.shift = a.shift; A.rtol = a.rtol; A.atol = a.atol;
    const ElimWork EW = projected_points(h, p, dZ, sigma, dmu, 1, st);
    // bytes as executed: the vectors each kernel reads and writes (mask, bounds and the optional outputs where given), the state bytes,
    // its partial results, and per workgroup the partial results it combines.  (Z and the bounds are read on free entries only; they
    // are counted whole.)
    const double v = 8.0 * (double)n, by = (double)n, m = a.mask ? v : 0.0, bounds = (a.lo ? v : 0.0) + (a.hi ? v : 0.0);
    const double outs = (a.zp ? v : 0.0) + (a.entry_state ? v : 0.0), part = 8.0 * (double)nb, groups = (double)((nb + 15) / 16);
    auto running = [&] {   // the one readback per iteration
        HIP_CHECK(hipMemcpyAsync(h->mailbox->newton, A.state, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return (int)h->mailbox->newton[NBS_STATUS] == NEWTON_CONTINUE;
    };
    { ProfScope ps(h, st, CAT_NEWTON_BOX, 5.0 * v + m + bounds + by + outs + 7.0 * part); launch_newton_box_start(st, R, A); }
    { ProfScope ps(h, st, CAT_NEWTON_BOX, (groups + 6.0) * part); launch_newton_box_dir(st, A, 0, a.max_iter); }
    for (int j = 1; j <= a.max_iter && running(); ++j) {
        projected_chunk(h, p, B, EW, store_route, dZ, 1, A.d, A.w, st, al);   // y = T'HT d (with `al`: T'(H + J_c' W J_c)T d)
        { ProfScope ps(h, st, CAT_NEWTON_BOX, 5.0 * v + bounds + by + 5.0 * part); launch_newton_box_curv(st, A); }
        { ProfScope ps(h, st, CAT_NEWTON_BOX, 8.0 * v + bounds + 2.0 * by + outs + 6.0 * part + groups * 5.0 * part); launch_newton_box_step(st, A, j); }
        { ProfScope ps(h, st, CAT_NEWTON_BOX, 3.0 * v + by + (2.0 * groups + 5.0) * part); launch_newton_box_dir(st, A, j, a.max_iter); }
    }
}

// The host-pointer form of the box step and, with `rho`, of dto_auglag_newton_step: upload, the device routine, download.
static int newton_box_host(dto_handle* h, const std::string& who, const double* Z, double sigma, const double* mu, const double* rho,
                           const double* free_mask, const double* lo, const double* hi, double radius, double shift, double rtol, double atol,
                           int32_t max_iter, double* p, double* info, double* trace, double* entry_state, double* Zp) {
    return guarded(h, [&] {
        const ElimPlan& ep = reduced_args(h, who, true);
        reduced_workspaces(h, ep);
        const size_t n = (size_t)h->n_vars, nt = NEWTON_BOX_TRACE * (size_t)max_iter, bytes = sizeof(double) * n;
        grow_workspace(h, h->d_newton_box, (size_t)newton_box_workspace_doubles(h->n_vars));   // before the uploads are enqueued
        block_workspaces(h, ep, 1, h->reduced_input_store && h->K >= 1);
        AlWork al{};
        if (rho) al = auglag_workspaces(h, 1);
        double* q = grow_workspace(h, h->d_newton_box_host, 6 * n + NEWTON_BOX_INFO + nt);
        double *dmask = q, *dlo = q + n, *dhi = q + 2 * n, *dp = q + 3 * n, *dzp = q + 4 * n, *des = q + 5 * n, *dinfo = q + 6 * n;
        double* dtrace = dinfo + NEWTON_BOX_INFO;
        upload_Z(h, Z);
        const bool has_mu = mu && h->n_cons > 0;
        if (has_mu) HIP_CHECK(hipMemcpyAsync(h->red_hmu, mu, sizeof(double) * (size_t)h->n_cons, hipMemcpyHostToDevice, h->stream));
        if (rho && h->n_cons > 0) HIP_CHECK(hipMemcpyAsync(al.hrho, rho, sizeof(double) * (size_t)h->n_cons, hipMemcpyHostToDevice, h->stream));
        if (free_mask) HIP_CHECK(hipMemcpyAsync(dmask, free_mask, bytes, hipMemcpyHostToDevice, h->stream));
        if (lo) HIP_CHECK(hipMemcpyAsync(dlo, lo, bytes, hipMemcpyHostToDevice, h->stream));
        if (hi) HIP_CHECK(hipMemcpyAsync(dhi, hi, bytes, hipMemcpyHostToDevice, h->stream));
        // the rows of the trace the step does not reach keep the caller's values
        if (trace) HIP_CHECK(hipMemcpyAsync(dtrace, trace, sizeof(double) * nt, hipMemcpyHostToDevice, h->stream));
        const NewtonBoxArgs a{free_mask ? dmask : nullptr, lo ? dlo : nullptr, hi ? dhi : nullptr, radius, shift, rtol, atol, max_iter, dp, dinfo,
                              trace ? dtrace : nullptr, entry_state ? des : nullptr, Zp ? dzp : nullptr};
        if (rho) {
            auglag_rows_at(h, al, h->d_Z, has_mu ? h->red_hmu : nullptr, al.hrho, nullptr, h->stream);
            newton_box_step(h, ep, h->d_Z, sigma, al.mu_eff, a, h->stream, &al);
        } else {
            newton_box_step(h, ep, h->d_Z, sigma, mu ? h->red_hmu : nullptr, a, h->stream);
        }
        HIP_CHECK(hipMemcpyAsync(p, dp, bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipMemcpyAsync(info, dinfo, sizeof(double) * NEWTON_BOX_INFO, hipMemcpyDeviceToHost, h->stream));
        if (trace) HIP_CHECK(hipMemcpyAsync(trace, dtrace, sizeof(double) * nt, hipMemcpyDeviceToHost, h->stream));
        if (entry_state) HIP_CHECK(hipMemcpyAsync(entry_state, des, bytes, hipMemcpyDeviceToHost, h->stream));
        if (Zp) HIP_CHECK(hipMemcpyAsync(Zp, dzp, bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}

int dto_projected_newton_step_box(dto_handle* h, const double* Z, double sigma, const double* mu, const double* free_mask, const double* lo,
                                  const double* hi, double radius, double shift, double rtol, double atol, int32_t max_iter, double* p,
                                  double* info, double* trace, double* entry_state, double* Zp) {
    const std::string who = "dto_projected_newton_step_box";
    if (!h) return fail(nullptr, "null handle");
    std::string bad = newton_refusal(who, Z, radius, shift, rtol, atol, max_iter, p, info);
    if (bad.empty()) bad = newton_box_refusal(who, (size_t)h->n_vars, Z, free_mask, lo, hi, p, Zp, entry_state);
    if (!bad.empty()) return fail(h, bad);
    return newton_box_host(h, who, Z, sigma, mu, nullptr, free_mask, lo, hi, radius, shift, rtol, atol, max_iter, p, info, trace, entry_state, Zp);
}
int dto_projected_newton_step_box_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* dfree_mask, const double* dlo,
                                      const double* dhi, double radius, double shift, double rtol, double atol, int32_t max_iter, double* dp,
                                      double* dinfo, double* dtrace, double* dentry_state, double* dZp, void* stream) {
    const std::string who = "dto_projected_newton_step_box_dev";
    if (!h) return fail(nullptr, "null handle");
    std::string bad = newton_refusal(who, dZ, radius, shift, rtol, atol, max_iter, dp, dinfo);
    if (bad.empty()) bad = newton_box_refusal(who, (size_t)h->n_vars, dZ, dfree_mask, dlo, dhi, dp, dZp, dentry_state);
    if (!bad.empty()) return fail(h, bad);
    return guarded(h, [&] {
        const ElimPlan& ep = reduced_args(h, who, true);
        reduced_workspaces(h, ep);
        const NewtonBoxArgs a{dfree_mask, dlo, dhi, radius, shift, rtol, atol, max_iter, dp, dinfo, dtrace, dentry_state, dZp};
        newton_box_step(h, ep, dZ, sigma, dmu, a, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}

int dto_projected_hessian_products(dto_handle* h, const double* Z, double sigma, const double* mu, int32_t n_cols, const double* V, double* Y) {
    return guarded(h, [&] {
        const std::string who = "dto_projected_hessian_products";
        const ElimPlan& p = reduced_args(h, who, true);
        block_args(who, n_cols, Z, V, Y);
        reduced_workspaces(h, p);
        const size_t n = (size_t)n_cols * (size_t)h->n_vars;
        double* dV = block_host_buffers(h, n_cols);
        block_workspaces(h, p, projected_width(h, n_cols), h->reduced_input_store && h->K >= 1);   // before the uploads are enqueued
        upload_Z(h, Z);
        if (mu && h->n_cons > 0) HIP_CHECK(hipMemcpyAsync(h->red_hmu, mu, sizeof(double) * (size_t)h->n_cons, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(dV, V, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
        projected_hessian_products(h, p, h->d_Z, sigma, mu ? h->red_hmu : nullptr, n_cols, dV, dV + n, h->stream);
        HIP_CHECK(hipMemcpyAsync(Y, dV + n, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_projected_hessian_products_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, int32_t n_cols, const double* dV,
                                       double* dY, void* stream) {
    return guarded(h, [&] {
        const std::string who = "dto_projected_hessian_products_dev";
        const ElimPlan& p = reduced_args(h, who, true);
        block_args(who, n_cols, dZ, dV, dY);
        reduced_workspaces(h, p);
        projected_hessian_products(h, p, dZ, sigma, dmu, n_cols, dV, dY, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}

// ---- feasible-trajectory rollout and reduced merit value (include/dto_engine.h, "Feasible trajectory"; dto_feasible.hip,
// dto_feasible_plan.h): the function the reduced-space operators are derivatives of.  A composition of do_jacobian, the rollout's tree
// and descent, do_objective and do_constraint, all on `st` and all unchanged; three small kernels keep the states on the device.

// What a feasible-trajectory call names: refused with text before anything is enqueued.
static const FeasiblePlan& feasible_args(dto_handle* h, const std::string& who, bool merit) {
    needs_unsharded(h, who);
    const ElimPlan& p = elim_plan_of(h);
    if (!p.refusal.empty()) throw HipError{who + ": " + p.refusal};
    if (merit) {
        if (h->n_ext_con + h->n_ext_obj > 0)
            throw HipError{who + ": the handle holds host-evaluated terms (" + std::to_string(h->n_ext_con) + " constraints, " +
                           std::to_string(h->n_ext_obj) + " objectives): the merit value runs on device-evaluated terms only"};
        int64_t rows = 0;
        for (size_t i = 0; i < h->integ_dim.size(); ++i) rows = std::max(rows, h->integ_row_off[i] + h->K * h->integ_dim[i]);
        if (h->n_dyn != h->K * p.n_states || rows > h->n_dyn) throw HipError{who + ": the dynamics rows are not the first (N - 1) n_states rows"};
    }
    if (!h->feas) {
        std::vector<int> propagates(p.level.size());
        for (size_t i = 0; i < p.level.size(); ++i) propagates[i] = elim_has_tree(h, (int)i) ? 1 : 0;
        h->feas.reset(new FeasiblePlan(feasible_plan(p.level, propagates)));
    }
    return *h->feas;
}

// the merit's block d_feas: Zf [n_vars], g [n_cons], the host-pointer form's mu [n_cons], f, phi
struct FeasWork { double *Zf, *g, *mu, *f, *phi; };

// Every workspace of a call, before anything is enqueued: the private slab, the rollout's tree and padded trajectory for the widest
// integrator with a propagator, and for the merit its own block.
static FeasWork feasible_workspaces(dto_handle* h, const FeasiblePlan& fp, bool merit) {
    int npad_max = 0;
    for (const FeasibleStep& s : fp.steps)
        if (s.kind == FEAS_ROLL) npad_max = std::max(npad_max, pad64(h->integ_dim[s.integrator]));
    if (npad_max && h->K >= 1) {
        jac_scratch(h);
        grow_workspace(h, h->d_roll_tree, rollout_tree_bytes(npad_max, h->K) / sizeof(double));
        grow_workspace(h, h->d_roll_S, rollout_traj_bytes(npad_max, h->K, 1) / sizeof(double));
    }
    FeasWork W{};
    if (!merit) return W;
    const size_t nv = (size_t)h->n_vars, nc = (size_t)std::max<int64_t>(h->n_cons, 1);
    double* q = grow_workspace(h, h->d_feas, nv + 2 * nc + 2);
    W.Zf = q; W.g = q + nv; W.mu = W.g + nc; W.f = W.mu + nc; W.phi = W.f + 1;
    return W;
}

// The device routine both entry-point families run: everything on `st`, dZ / dZf device pointers, dZf == dZ works in place.
static void feasible_trajectory(dto_handle* h, const FeasiblePlan& fp, const double* dZ, double* dZf, hipStream_t st) {
    const int64_t K = h->K;
    if (dZf != dZ) HIP_CHECK(hipMemcpyAsync(dZf, dZ, sizeof(double) * (size_t)h->n_vars, hipMemcpyDeviceToDevice, st));
    if (K < 1) return;   // a single knot: the copy
    double* slab = nullptr;
    for (const FeasibleStep& s : fp.steps) {
        if (s.kind == FEAS_DERIV) {
            const KDer& d = h->der[h->integ_index[s.integrator]];
            ProfScope ps(h, st, CAT_FEASIBLE, 8.0 * (double)K * (2.0 * d.d + 1.0) + 8.0 * (double)(K + 1) * d.d);
            launch_feas_deriv(st, K, h->z, h->dt_idx, d, dZf);
            continue;
        }
        if (s.kind == FEAS_JACOBIAN) {
            // the whole Jacobian at the trajectory built so far, once per level: the x_k columns of every integrator of the level then
            // hold -E_k.  (The tree the single-integrator solves keep per point shares the workspaces below and is overwritten.)
            h->dyn_point.rec.drop();
            slab = jac_scratch(h);
            do_jacobian(h, dZf, slab, st);
            continue;
        }
        const KRollout R = rollout_args(h, s.integrator, 1, DTO_ROLLOUT_ALL, false, "dto_feasible_trajectory");
        double* tree = h->d_roll_tree.p;
        double* S = h->d_roll_S.p;
        rollout_tree_from_slab(h, R, slab, tree, st, CAT_ROLLOUT, CAT_ROLLOUT_TREE);
        { ProfScope ps(h, st, CAT_ROLLOUT_DESCENT, 0.0); launch_rollout_start(st, R, dZf, nullptr, S); }
        const double item_flops = 2.0 * (double)R.npad * R.npad * R.col_pad;
        for (int l = R.L + 1; l >= 1; --l) {
            const int64_t live = dynsolve_live_items(R.L, K, 0, l);
            if (live == 0) continue;
            ProfScope ps(h, st, CAT_ROLLOUT_DESCENT, item_flops * (double)live);
            launch_rollout_descend(st, R, l, -1, tree, S);
        }
        ProfScope ps(h, st, CAT_FEASIBLE, 16.0 * (double)K * R.n);
        launch_feas_scatter(st, R, h->z, S, dZf);
    }
}

// phi = sigma f(Zf) + sum over the non-dynamics rows of mu_r g_r(Zf), Zf = the feasible trajectory of dZ.  dZf / dg null: the
// workspace's (g is evaluated only where dg or dmu asks for it).
static void feasible_merit(dto_handle* h, const FeasiblePlan& fp, const FeasWork& W, const double* dZ, double sigma, const double* dmu,
                           double* dphi, double* dZf, double* dg, hipStream_t st) {
    double* Zf = dZf ? dZf : W.Zf;
    feasible_trajectory(h, fp, dZ, Zf, st);
    do_objective(h, Zf, W.f, st);
    double* g = dg ? dg : W.g;
    if (dg || dmu) do_constraint(h, Zf, g, st);
    ProfScope ps(h, st, CAT_FEASIBLE, 16.0 + (dmu ? 16.0 * (double)(h->n_cons - h->n_dyn) : 0.0));
    launch_feas_merit(st, h->n_dyn, h->n_cons, sigma, W.f, dmu, g, dphi);
}

int dto_feasible_trajectory(dto_handle* h, const double* Z, double* Zf) {
    return guarded(h, [&] {
        const std::string who = "dto_feasible_trajectory";
        const FeasiblePlan& fp = feasible_args(h, who, false);
        if (!Z || !Zf) throw HipError{who + ": Z and Zf are required (NULL given)"};
        feasible_workspaces(h, fp, false);
        upload_Z(h, Z);
        feasible_trajectory(h, fp, h->d_Z, h->d_Z, h->stream);   // in place in the handle's copy
        HIP_CHECK(hipMemcpyAsync(Zf, h->d_Z, sizeof(double) * (size_t)h->n_vars, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_feasible_trajectory_dev(dto_handle* h, const double* dZ, double* dZf, void* stream) {
    return guarded(h, [&] {
        const std::string who = "dto_feasible_trajectory_dev";
        const FeasiblePlan& fp = feasible_args(h, who, false);
        if (!dZ || !dZf) throw HipError{who + ": dZ and dZf are required (NULL given)"};
        feasible_workspaces(h, fp, false);
        feasible_trajectory(h, fp, dZ, dZf, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}
int dto_feasible_merit(dto_handle* h, const double* Z, double sigma, const double* mu, double* phi, double* Zf, double* g) {
    return guarded(h, [&] {
        const std::string who = "dto_feasible_merit";
        const FeasiblePlan& fp = feasible_args(h, who, true);
        if (!Z || !phi) throw HipError{who + ": Z and phi are required (NULL given)"};
        const FeasWork W = feasible_workspaces(h, fp, true);
        upload_Z(h, Z);
        const bool has_mu = mu && h->n_cons > 0;
        if (has_mu) HIP_CHECK(hipMemcpyAsync(W.mu, mu, sizeof(double) * (size_t)h->n_cons, hipMemcpyHostToDevice, h->stream));
        feasible_merit(h, fp, W, h->d_Z, sigma, has_mu ? W.mu : nullptr, W.phi, h->d_Z, g ? W.g : nullptr, h->stream);
        HIP_CHECK(hipMemcpyAsync(phi, W.phi, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (Zf) HIP_CHECK(hipMemcpyAsync(Zf, h->d_Z, sizeof(double) * (size_t)h->n_vars, hipMemcpyDeviceToHost, h->stream));
        if (g && h->n_cons > 0) HIP_CHECK(hipMemcpyAsync(g, W.g, sizeof(double) * (size_t)h->n_cons, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_feasible_merit_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, double* dphi, double* dZf, double* dg, void* stream) {
    return guarded(h, [&] {
        const std::string who = "dto_feasible_merit_dev";
        const FeasiblePlan& fp = feasible_args(h, who, true);
        if (!dZ || !dphi) throw HipError{who + ": dZ and dphi are required (NULL given)"};
        const FeasWork W = feasible_workspaces(h, fp, true);
        feasible_merit(h, fp, W, dZ, sigma, h->n_cons > 0 ? dmu : nullptr, dphi, dZf, dg, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}

// ---- augmented-Lagrangian entry points (include/dto_engine.h, "Augmented-Lagrangian terms").  Each call extends one of the calls above;
// with rho == NULL it IS that call.

static bool spans_overlap(const double* a, size_t na, const double* b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb * sizeof(double) && y < x + na * sizeof(double);
}

struct AlSpan { const char* name; const double* p; size_t n; };

// What every dto_auglag_* call names before the handle is touched: host-evaluated constraints, in the host-pointer forms a penalty that
// is negative or a NaN, and outputs that overlap inputs.
static std::string auglag_refusal(const dto_handle* h, const std::string& who, const double* rho_host, std::initializer_list<AlSpan> outs,
                                  std::initializer_list<AlSpan> ins) {
    if (h->n_ext_con > 0)
        return who + ": the handle holds " + std::to_string(h->n_ext_con) +
               " host-evaluated constraint(s) (global constraints are among these): the augmented-Lagrangian terms run on device-evaluated constraints only";
    if (rho_host)
        for (int64_t r = h->n_dyn; r < h->n_cons; ++r)
            if (!(rho_host[r] >= 0.0))
                return who + ": rho[" + std::to_string(r) + "] = " + std::to_string(rho_host[r]) + " (row " + std::to_string(r) +
                       "): a penalty must be >= 0 and no NaN";
    for (const AlSpan& o : outs)
        for (const AlSpan& i : ins)
            if (spans_overlap(o.p, o.n, i.p, i.n)) return who + ": " + o.name + " overlaps " + i.name;
    return "";
}

// what a row pass names beyond that
static void auglag_rows_args(dto_handle* h, const std::string& who) {
    needs_unsharded(h, who);
    if (h->n_ext_int > 0) throw HipError{who + ": the handle holds host-evaluated integrators: the row pass runs on device-evaluated terms only"};
}

int dto_auglag_rows(dto_handle* h, const double* Z, const double* mu, const double* rho, double* mu_eff, double* weight, double* info) {
    const std::string who = "dto_auglag_rows";
    if (!h) return fail(nullptr, "null handle");
    if (!Z) return fail(h, who + ": Z is required (NULL given)");
    const size_t nc = (size_t)h->n_cons, nv = (size_t)h->n_vars;
    const std::string bad = auglag_refusal(h, who, rho, {{"mu_eff", mu_eff, nc}, {"weight", weight, nc}, {"info", info, AL_INFO}},
                                           {{"Z", Z, nv}, {"mu", mu, nc}, {"rho", rho, nc}});
    if (!bad.empty()) return fail(h, bad);
    return guarded(h, [&] {
        auglag_rows_args(h, who);
        const AlWork A = auglag_workspaces(h, 0);
        upload_Z(h, Z);
        const bool has_mu = mu && nc > 0, has_rho = rho && nc > 0;
        if (has_mu) HIP_CHECK(hipMemcpyAsync(A.hmu, mu, sizeof(double) * nc, hipMemcpyHostToDevice, h->stream));
        if (has_rho) HIP_CHECK(hipMemcpyAsync(A.hrho, rho, sizeof(double) * nc, hipMemcpyHostToDevice, h->stream));
        auglag_rows_at(h, A, h->d_Z, has_mu ? A.hmu : nullptr, has_rho ? A.hrho : nullptr, A.info, h->stream);
        if (mu_eff && nc > 0) HIP_CHECK(hipMemcpyAsync(mu_eff, A.mu_eff, sizeof(double) * nc, hipMemcpyDeviceToHost, h->stream));
        if (weight && nc > 0) HIP_CHECK(hipMemcpyAsync(weight, A.weight, sizeof(double) * nc, hipMemcpyDeviceToHost, h->stream));
        if (info) HIP_CHECK(hipMemcpyAsync(info, A.info, sizeof(double) * AL_INFO, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_auglag_rows_dev(dto_handle* h, const double* dZ, const double* dmu, const double* drho, double* dmu_eff, double* dweight, double* dinfo,
                        void* stream) {
    const std::string who = "dto_auglag_rows_dev";
    if (!h) return fail(nullptr, "null handle");
    if (!dZ) return fail(h, who + ": dZ is required (NULL given)");
    const size_t nc = (size_t)h->n_cons, nv = (size_t)h->n_vars;
    const std::string bad = auglag_refusal(h, who, nullptr, {{"dmu_eff", dmu_eff, nc}, {"dweight", dweight, nc}, {"dinfo", dinfo, AL_INFO}},
                                           {{"dZ", dZ, nv}, {"dmu", dmu, nc}, {"drho", drho, nc}});
    if (!bad.empty()) return fail(h, bad);
    return guarded(h, [&] {
        auglag_rows_args(h, who);
        const AlWork A = auglag_workspaces(h, 0);
        hipStream_t st = (hipStream_t)stream;
        for (auto& c : h->con) launch_cons_knot(st, h->P, c.k, dZ, A.g);
        auglag_row_pass(h, A.g, dmu, drho, dmu_eff, dweight, dinfo, 0.0, nullptr, nullptr, st);
    }, G_ASYNC, (hipStream_t)stream);
}

int dto_auglag_merit(dto_handle* h, const double* Z, double sigma, const double* mu, const double* rho, double* phi, double* Zf, double* g,
                     double* info) {
    const std::string who = "dto_auglag_merit";
    if (!h) return fail(nullptr, "null handle");
    const size_t nc = (size_t)h->n_cons, nv = (size_t)h->n_vars;
    const std::string bad = auglag_refusal(h, who, rho, {{"phi", phi, 1}, {"Zf", Zf, nv}, {"g", g, nc}, {"info", info, AL_INFO}},
                                           {{"Z", Z, nv}, {"mu", mu, nc}, {"rho", rho, nc}});
    if (!bad.empty()) return fail(h, bad);
    if (!rho) return dto_feasible_merit(h, Z, sigma, mu, phi, Zf, g);
    return guarded(h, [&] {
        const FeasiblePlan& fp = feasible_args(h, who, true);
        if (!Z || !phi) throw HipError{who + ": Z and phi are required (NULL given)"};
        const FeasWork W = feasible_workspaces(h, fp, true);
        const AlWork A = auglag_workspaces(h, 0);
        upload_Z(h, Z);
        const bool has_mu = mu && nc > 0;
        if (has_mu) HIP_CHECK(hipMemcpyAsync(W.mu, mu, sizeof(double) * nc, hipMemcpyHostToDevice, h->stream));
        if (nc > 0) HIP_CHECK(hipMemcpyAsync(A.hrho, rho, sizeof(double) * nc, hipMemcpyHostToDevice, h->stream));
        feasible_trajectory(h, fp, h->d_Z, h->d_Z, h->stream);
        do_objective(h, h->d_Z, W.f, h->stream);
        do_constraint(h, h->d_Z, W.g, h->stream);
        auglag_row_pass(h, W.g, has_mu ? W.mu : nullptr, A.hrho, nullptr, nullptr, A.info, sigma, W.f, W.phi, h->stream);
        HIP_CHECK(hipMemcpyAsync(phi, W.phi, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (Zf) HIP_CHECK(hipMemcpyAsync(Zf, h->d_Z, sizeof(double) * nv, hipMemcpyDeviceToHost, h->stream));
        if (g && nc > 0) HIP_CHECK(hipMemcpyAsync(g, W.g, sizeof(double) * nc, hipMemcpyDeviceToHost, h->stream));
        if (info) HIP_CHECK(hipMemcpyAsync(info, A.info, sizeof(double) * AL_INFO, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_auglag_merit_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* drho, double* dphi, double* dZf, double* dg,
                         double* dinfo, void* stream) {
    const std::string who = "dto_auglag_merit_dev";
    if (!h) return fail(nullptr, "null handle");
    const size_t nc = (size_t)h->n_cons, nv = (size_t)h->n_vars;
    const std::string bad = auglag_refusal(h, who, nullptr, {{"dphi", dphi, 1}, {"dZf", dZf, nv}, {"dg", dg, nc}, {"dinfo", dinfo, AL_INFO}},
                                           {{"dmu", dmu, nc}, {"drho", drho, nc}});   // (dZf == dZ works in place, as in dto_feasible_merit_dev)
    if (!bad.empty()) return fail(h, bad);
    if (!drho) return dto_feasible_merit_dev(h, dZ, sigma, dmu, dphi, dZf, dg, stream);
    return guarded(h, [&] {
        const FeasiblePlan& fp = feasible_args(h, who, true);
        if (!dZ || !dphi) throw HipError{who + ": dZ and dphi are required (NULL given)"};
        const FeasWork W = feasible_workspaces(h, fp, true);
        auglag_workspaces(h, 0);
        hipStream_t st = (hipStream_t)stream;
        double* Zf = dZf ? dZf : W.Zf;
        double* gg = dg ? dg : W.g;
        feasible_trajectory(h, fp, dZ, Zf, st);
        do_objective(h, Zf, W.f, st);
        do_constraint(h, Zf, gg, st);
        auglag_row_pass(h, gg, nc > 0 ? dmu : nullptr, drho, nullptr, nullptr, dinfo, sigma, W.f, dphi, st);
    }, G_ASYNC, (hipStream_t)stream);
}

int dto_auglag_gradient(dto_handle* h, const double* Z, double sigma, const double* mu, const double* rho, double* grad, double* lam, double* mu_eff) {
    const std::string who = "dto_auglag_gradient";
    if (!h) return fail(nullptr, "null handle");
    const size_t nc = (size_t)h->n_cons, nv = (size_t)h->n_vars;
    const std::string bad = auglag_refusal(h, who, rho, {{"grad", grad, nv}, {"mu_eff", mu_eff, nc}}, {{"Z", Z, nv}, {"mu", mu, nc}, {"rho", rho, nc}});
    if (!bad.empty()) return fail(h, bad);
    if (!rho) {   // no penalties: the call it extends; mu_eff is mu with its dynamics rows zeroed
        const int rc = dto_reduced_gradient(h, Z, sigma, mu, grad, lam);
        if (rc == 0 && mu_eff)
            for (int64_t r = 0; r < h->n_cons; ++r) mu_eff[r] = (mu && r >= h->n_dyn) ? mu[r] : 0.0;
        return rc;
    }
    return guarded(h, [&] {
        const ElimPlan& p = reduced_args(h, who, false);
        if (!Z || !grad) throw HipError{who + ": Z and grad are required (NULL given)"};
        reduced_workspaces(h, p);
        const AlWork A = auglag_workspaces(h, 0);
        upload_Z(h, Z);
        const bool has_mu = mu && nc > 0;
        if (has_mu) HIP_CHECK(hipMemcpyAsync(h->red_hmu, mu, sizeof(double) * nc, hipMemcpyHostToDevice, h->stream));
        if (nc > 0) HIP_CHECK(hipMemcpyAsync(A.hrho, rho, sizeof(double) * nc, hipMemcpyHostToDevice, h->stream));
        auglag_rows_at(h, A, h->d_Z, has_mu ? h->red_hmu : nullptr, A.hrho, nullptr, h->stream);
        reduced_point(h, p, h->d_Z, sigma, A.mu_eff, h->stream);
        HIP_CHECK(hipMemcpyAsync(grad, h->red_r, sizeof(double) * nv, hipMemcpyDeviceToHost, h->stream));
        if (lam) HIP_CHECK(hipMemcpyAsync(lam, h->red_lam, sizeof(double) * (size_t)h->N * p.n_states, hipMemcpyDeviceToHost, h->stream));
        if (mu_eff && nc > 0) HIP_CHECK(hipMemcpyAsync(mu_eff, A.mu_eff, sizeof(double) * nc, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_auglag_gradient_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* drho, double* dgrad, double* dlam,
                            double* dmu_eff, void* stream) {
    const std::string who = "dto_auglag_gradient_dev";
    if (!h) return fail(nullptr, "null handle");
    const size_t nc = (size_t)h->n_cons, nv = (size_t)h->n_vars;
    const std::string bad = auglag_refusal(h, who, nullptr, {{"dgrad", dgrad, nv}, {"dmu_eff", dmu_eff, nc}},
                                           {{"dZ", dZ, nv}, {"dmu", dmu, nc}, {"drho", drho, nc}});
    if (!bad.empty()) return fail(h, bad);
    if (!drho) {
        const int rc = dto_reduced_gradient_dev(h, dZ, sigma, dmu, dgrad, dlam, stream);
        if (rc != 0 || !dmu_eff || nc == 0) return rc;
        return guarded(h, [&] {   // copies, no launch
            hipStream_t st = (hipStream_t)stream;
            const size_t nd = (size_t)h->n_dyn;
            HIP_CHECK(hipMemsetAsync(dmu_eff, 0, sizeof(double) * (dmu ? nd : nc), st));
            if (dmu && nc > nd) HIP_CHECK(hipMemcpyAsync(dmu_eff + nd, dmu + nd, sizeof(double) * (nc - nd), hipMemcpyDeviceToDevice, st));
        }, G_ASYNC, (hipStream_t)stream);
    }
    return guarded(h, [&] {
        const ElimPlan& p = reduced_args(h, who, false);
        if (!dZ || !dgrad) throw HipError{who + ": dZ and dgrad are required (NULL given)"};
        reduced_workspaces(h, p);
        const AlWork A = auglag_workspaces(h, 0);
        hipStream_t st = (hipStream_t)stream;
        auglag_rows_at(h, A, dZ, nc > 0 ? dmu : nullptr, drho, nullptr, st);
        reduced_gradient(h, p, dZ, sigma, A.mu_eff, dgrad, dlam, st);
        if (dmu_eff && nc > 0) HIP_CHECK(hipMemcpyAsync(dmu_eff, A.mu_eff, sizeof(double) * nc, hipMemcpyDeviceToDevice, st));
    }, G_ASYNC, (hipStream_t)stream);
}

int dto_auglag_hessian_products(dto_handle* h, const double* Z, double sigma, const double* mu, const double* rho, int32_t n_cols, const double* V,
                                double* Y) {
    const std::string who = "dto_auglag_hessian_products";
    if (!h) return fail(nullptr, "null handle");
    const size_t nc = (size_t)h->n_cons, nv = (size_t)h->n_vars, nb = (size_t)std::max(n_cols, 0) * nv;
    const std::string bad = auglag_refusal(h, who, rho, {{"Y", Y, nb}}, {{"Z", Z, nv}, {"mu", mu, nc}, {"rho", rho, nc}, {"V", V, nb}});
    if (!bad.empty()) return fail(h, bad);
    if (!rho) return dto_projected_hessian_products(h, Z, sigma, mu, n_cols, V, Y);
    return guarded(h, [&] {
        const ElimPlan& p = reduced_args(h, who, true);
        block_args(who, n_cols, Z, V, Y);
        reduced_workspaces(h, p);
        double* dV = block_host_buffers(h, n_cols);
        block_workspaces(h, p, projected_width(h, n_cols), h->reduced_input_store && h->K >= 1);   // before the uploads are enqueued
        const AlWork A = auglag_workspaces(h, projected_width(h, n_cols));
        upload_Z(h, Z);
        const bool has_mu = mu && nc > 0;
        if (has_mu) HIP_CHECK(hipMemcpyAsync(h->red_hmu, mu, sizeof(double) * nc, hipMemcpyHostToDevice, h->stream));
        if (nc > 0) HIP_CHECK(hipMemcpyAsync(A.hrho, rho, sizeof(double) * nc, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(dV, V, sizeof(double) * nb, hipMemcpyHostToDevice, h->stream));
        auglag_rows_at(h, A, h->d_Z, has_mu ? h->red_hmu : nullptr, A.hrho, nullptr, h->stream);
        projected_hessian_products(h, p, h->d_Z, sigma, A.mu_eff, n_cols, dV, dV + nb, h->stream, &A);
        HIP_CHECK(hipMemcpyAsync(Y, dV + nb, sizeof(double) * nb, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_auglag_hessian_products_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* drho, int32_t n_cols,
                                    const double* dV, double* dY, void* stream) {
    const std::string who = "dto_auglag_hessian_products_dev";
    if (!h) return fail(nullptr, "null handle");
    const size_t nc = (size_t)h->n_cons, nv = (size_t)h->n_vars, nb = (size_t)std::max(n_cols, 0) * nv;
    const std::string bad = auglag_refusal(h, who, nullptr, {{"dY", dY, nb}}, {{"dZ", dZ, nv}, {"dmu", dmu, nc}, {"drho", drho, nc}, {"dV", dV, nb}});
    if (!bad.empty()) return fail(h, bad);
    if (!drho) return dto_projected_hessian_products_dev(h, dZ, sigma, dmu, n_cols, dV, dY, stream);
    return guarded(h, [&] {
        const ElimPlan& p = reduced_args(h, who, true);
        block_args(who, n_cols, dZ, dV, dY);
        reduced_workspaces(h, p);
        const int W = projected_width(h, n_cols);
        block_workspaces(h, p, W, h->reduced_input_store && h->K >= 1);
        const AlWork A = auglag_workspaces(h, W);
        hipStream_t st = (hipStream_t)stream;
        auglag_rows_at(h, A, dZ, nc > 0 ? dmu : nullptr, drho, nullptr, st);
        projected_hessian_products(h, p, dZ, sigma, A.mu_eff, n_cols, dV, dY, st, &A);
    }, G_ASYNC, (hipStream_t)stream);
}

int dto_auglag_newton_step(dto_handle* h, const double* Z, double sigma, const double* mu, const double* rho, const double* free_mask,
                           const double* lo, const double* hi, double radius, double shift, double rtol, double atol, int32_t max_iter, double* p,
                           double* info, double* trace, double* entry_state, double* Zp) {
    const std::string who = "dto_auglag_newton_step";
    if (!h) return fail(nullptr, "null handle");
    std::string bad = newton_refusal(who, Z, radius, shift, rtol, atol, max_iter, p, info);
    if (bad.empty()) bad = newton_box_refusal(who, (size_t)h->n_vars, Z, free_mask, lo, hi, p, Zp, entry_state);
    const size_t nc = (size_t)h->n_cons, nv = (size_t)h->n_vars;
    if (bad.empty())
        bad = auglag_refusal(h, who, rho, {{"p", p, nv}, {"Zp", Zp, nv}, {"entry_state", entry_state, nv}, {"info", info, NEWTON_BOX_INFO}},
                             {{"mu", mu, nc}, {"rho", rho, nc}});
    if (!bad.empty()) return fail(h, bad);
    return newton_box_host(h, rho ? who : std::string("dto_projected_newton_step_box"), Z, sigma, mu, rho, free_mask, lo, hi, radius, shift, rtol, atol,
                           max_iter, p, info, trace, entry_state, Zp);
}
int dto_auglag_newton_step_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* drho, const double* dfree_mask,
                               const double* dlo, const double* dhi, double radius, double shift, double rtol, double atol, int32_t max_iter,
                               double* dp, double* dinfo, double* dtrace, double* dentry_state, double* dZp, void* stream) {
    const std::string who = "dto_auglag_newton_step_dev";
    if (!h) return fail(nullptr, "null handle");
    std::string bad = newton_refusal(who, dZ, radius, shift, rtol, atol, max_iter, dp, dinfo);
    if (bad.empty()) bad = newton_box_refusal(who, (size_t)h->n_vars, dZ, dfree_mask, dlo, dhi, dp, dZp, dentry_state);
    const size_t nc = (size_t)h->n_cons, nv = (size_t)h->n_vars;
    if (bad.empty())
        bad = auglag_refusal(h, who, nullptr, {{"dp", dp, nv}, {"dZp", dZp, nv}, {"dentry_state", dentry_state, nv}, {"dinfo", dinfo, NEWTON_BOX_INFO}},
                             {{"dmu", dmu, nc}, {"drho", drho, nc}});
    if (!bad.empty()) return fail(h, bad);
    if (!drho)
        return dto_projected_newton_step_box_dev(h, dZ, sigma, dmu, dfree_mask, dlo, dhi, radius, shift, rtol, atol, max_iter, dp, dinfo, dtrace,
                                                 dentry_state, dZp, stream);
    return guarded(h, [&] {
        const ElimPlan& ep = reduced_args(h, who, true);
        reduced_workspaces(h, ep);
        grow_workspace(h, h->d_newton_box, (size_t)newton_box_workspace_doubles(h->n_vars));   // before the row pass is enqueued
        block_workspaces(h, ep, 1, h->reduced_input_store && h->K >= 1);
        const AlWork A = auglag_workspaces(h, 1);
        hipStream_t st = (hipStream_t)stream;
        auglag_rows_at(h, A, dZ, nc > 0 ? dmu : nullptr, drho, nullptr, st);
        const NewtonBoxArgs a{dfree_mask, dlo, dhi, radius, shift, rtol, atol, max_iter, dp, dinfo, dtrace, dentry_state, dZp};
        newton_box_step(h, ep, dZ, sigma, A.mu_eff, a, st, &A);
    }, G_ASYNC, (hipStream_t)stream);
}

// ---- L-BFGS-preconditioned truncated-Newton step (include/dto_engine.h, "Preconditioned truncated-Newton step"; dto_precond.hip,
// dto_precond_plan.h): newton_box_step's shape with z = P H P r behind the start and behind every update, the pairs in a two-bank store
// on the handle.

// The kernels' record over the routine's workspace and the store as it stands.  The workspace is sized for the capacity, so it is
// allocated once per option value; the store is allocated whole where a pair may be written.
static KPrecond precond_kernel_args(dto_handle* h, bool writes_pairs) {
    const int64_t n = h->n_vars, nb = newton_chunks(n);
    const int m = h->newton_pairs, cnt = h->pairs_count;
    double* q = grow_workspace(h, h->d_precond, (size_t)precond_workspace_doubles(n, m));
    if (writes_pairs) grow_workspace(h, h->d_pairs, (size_t)precond_store_doubles(n, m));
    KPrecond K{};
    KNewtonBox& A = K.B;
    A.n = n; A.nb = nb;
    A.r = q; A.d = q + n; A.w = q + 2 * n; K.z = q + 3 * n;
    A.part = q + 4 * n;
    K.uv = A.part + PRECOND_SLOTS * nb;
    K.gram = K.uv + 2 * (int64_t)cnt * nb;
    A.state = K.gram + (int64_t)precond_gram_count(cnt) * nb;
    K.pc = A.state + PRECOND_STATE;
    A.es = (unsigned char*)(K.pc + PRECOND_PC);
    K.m = m; K.head = h->pairs_head; K.cnt = cnt; K.harvest = 0;
    if (h->d_pairs.p && m > 0) {
        const size_t bank = 2 * (size_t)m * (size_t)n;
        K.S = h->d_pairs.p + (size_t)h->pairs_bank * bank;
        K.Y = K.S + (size_t)m * (size_t)n;
        K.HS = h->d_pairs.p + (size_t)(h->pairs_bank ^ 1) * bank;
        K.HY = K.HS + (size_t)m * (size_t)n;
    }
    return K;
}

// the preparation behind the entry states, and the application to r behind the start (or to a column of dto_newton_precondition)
static void precond_prepare_launches(dto_handle* h, const KPrecond& K, hipStream_t st) {
    if (K.cnt == 0) return;
    const double v = 8.0 * (double)K.B.n, part = 8.0 * (double)K.B.nb, g = (double)precond_gram_count(K.cnt);
    { ProfScope ps(h, st, CAT_PRECOND, 2.0 * K.cnt * v + (double)K.B.n + g * part); launch_precond_gram(st, K); }
    { ProfScope ps(h, st, CAT_PRECOND, g * part + 8.0 * PRECOND_PC); launch_precond_prep(st, K); }
}
static void precond_apply_launches(dto_handle* h, const KPrecond& K, const double* r, double* z, int j, bool dots, hipStream_t st) {
    const double v = 8.0 * (double)K.B.n, by = (double)K.B.n, part = 8.0 * (double)K.B.nb, groups = (double)((K.B.nb + 15) / 16);
    if (dots && K.cnt > 0) { ProfScope ps(h, st, CAT_PRECOND, (2.0 * K.cnt + 1.0) * v + by + 2.0 * K.cnt * part); launch_precond_dots(st, K, r); }
    ProfScope ps(h, st, CAT_PRECOND, (2.0 * K.cnt + 2.0) * v + by + part + groups * (2.0 * K.cnt * part + 8.0 * PRECOND_PC));
    launch_precond_comb(st, K, r, z, j);
}

// The device routine both entry-point families run: everything on `st`, every pointer a device pointer.
static void precond_step(dto_handle* h, const ElimPlan& p, const double* dZ, double sigma, const double* dmu, const NewtonBoxArgs& a, int harvest,
                         hipStream_t st, const AlWork* al = nullptr) {
    const KReduced& R = h->red;
    const bool store_route = h->reduced_input_store && h->K >= 1;
    // every workspace before anything is enqueued
    KPrecond K = precond_kernel_args(h, harvest != 0);
    const BlockWork B = block_workspaces(h, p, 1, store_route);
    KNewtonBox& A = K.B;
    K.harvest = harvest ? 1 : 0;
    A.p = a.p; A.g = h->red_r; A.mask = a.mask; A.Z = dZ; A.lo = a.lo; A.hi = a.hi;
    A.info = a.info; A.trace = a.trace; A.zp = a.zp; A.es_out = a.entry_state;
    A.radius = a.radius; A.shift = a.shift; A.rtol = a.rtol; A.atol = a.atol;
    const ElimWork EW = projected_points(h, p, dZ, sigma, dmu, 1, st);
    const int64_t nb = A.nb;
    const double v = 8.0 * (double)A.n, by = (double)A.n, m = a.mask ? v : 0.0, bounds = (a.lo ? v : 0.0) + (a.hi ? v : 0.0);
    const double outs = (a.zp ? v : 0.0) + (a.entry_state ? v : 0.0), part = 8.0 * (double)nb, groups = (double)((nb + 15) / 16);
    const double pairs = 2.0 * K.cnt;
    auto read_back = [&] {   // the one readback per iteration: status, iterations, pairs taken
        HIP_CHECK(hipMemcpyAsync(h->mailbox->precond, A.state, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return (int)h->mailbox->precond[NPS_STATUS] == NEWTON_CONTINUE;
    };
    { ProfScope ps(h, st, CAT_PRECOND, 5.0 * v + m + bounds + by + outs + 7.0 * part); launch_newton_box_start(st, R, A); }
    precond_prepare_launches(h, K, st);
    precond_apply_launches(h, K, A.r, K.z, 0, true, st);
    { ProfScope ps(h, st, CAT_PRECOND, 2.0 * v + by + (3.0 * groups + 5.0) * part); launch_precond_dir(st, K, 0, a.max_iter); }
    for (int j = 1; j <= a.max_iter && read_back(); ++j) {
        projected_chunk(h, p, B, EW, store_route, dZ, 1, A.d, A.w, st, al);   // y = T'HT d (with `al`: T'(H + J_c' W J_c)T d)
        { ProfScope ps(h, st, CAT_PRECOND, 5.0 * v + bounds + by + 5.0 * part); launch_newton_box_curv(st, A); }
        {   // the box step's bytes, the harvest copy where a pair may be taken, the multi-dot pass (counted as if the preconditioner is on)
            ProfScope ps(h, st, CAT_PRECOND,
                         (8.0 + (harvest ? 2.0 : 0.0) + pairs) * v + bounds + 2.0 * by + outs + (6.0 + pairs) * part + groups * 5.0 * part);
            launch_precond_step(st, K, j);
        }
        precond_apply_launches(h, K, A.r, K.z, j, false, st);
        { ProfScope ps(h, st, CAT_PRECOND, 3.0 * v + by + (3.0 * groups + 5.0) * part); launch_precond_dir(st, K, j, a.max_iter); }
    }
    if (!harvest) return;
    read_back();
    const int64_t taken = (int64_t)h->mailbox->precond[NPS_TAKEN_OUT];
    if (taken < 1) return;
    h->pairs_bank ^= 1;
    h->pairs_count = (int)std::min<int64_t>(K.m, taken);
    h->pairs_head = taken > K.m ? (int)(taken % K.m) : 0;
}

static std::string precond_refusal(const dto_handle* h, const std::string& who, int32_t harvest) {
    if (harvest != 0 && h->newton_pairs == 0)
        return who + ": harvest needs a pair store: set the option newton_pairs to 1 .. " + std::to_string(PRECOND_MAX_PAIRS) + " first (it is 0)";
    return "";
}

int dto_preconditioned_newton_step(dto_handle* h, const double* Z, double sigma, const double* mu, const double* rho, const double* free_mask,
                                   const double* lo, const double* hi, double radius, double shift, double rtol, double atol, int32_t max_iter,
                                   int32_t harvest, double* p, double* info, double* trace, double* entry_state, double* Zp) {
    const std::string who = "dto_preconditioned_newton_step";
    if (!h) return fail(nullptr, "null handle");
    std::string bad = newton_refusal(who, Z, radius, shift, rtol, atol, max_iter, p, info);
    if (bad.empty()) bad = newton_box_refusal(who, (size_t)h->n_vars, Z, free_mask, lo, hi, p, Zp, entry_state);
    const size_t nc = (size_t)h->n_cons, nv = (size_t)h->n_vars;
    if (bad.empty() && rho)
        bad = auglag_refusal(h, who, rho, {{"p", p, nv}, {"Zp", Zp, nv}, {"entry_state", entry_state, nv}, {"info", info, PRECOND_INFO}},
                             {{"mu", mu, nc}, {"rho", rho, nc}});
    if (bad.empty()) bad = precond_refusal(h, who, harvest);
    if (!bad.empty()) return fail(h, bad);
    return guarded(h, [&] {
        const ElimPlan& ep = reduced_args(h, who, true);
        reduced_workspaces(h, ep);
        const size_t n = (size_t)h->n_vars, nt = PRECOND_TRACE * (size_t)max_iter, bytes = sizeof(double) * n;
        precond_kernel_args(h, harvest != 0);   // before the uploads are enqueued
        block_workspaces(h, ep, 1, h->reduced_input_store && h->K >= 1);
        AlWork al{};
        if (rho) al = auglag_workspaces(h, 1);
        double* q = grow_workspace(h, h->d_precond_host, 6 * n + PRECOND_INFO + nt);
        double *dmask = q, *dlo = q + n, *dhi = q + 2 * n, *dp = q + 3 * n, *dzp = q + 4 * n, *des = q + 5 * n, *dinfo = q + 6 * n;
        double* dtrace = dinfo + PRECOND_INFO;
        upload_Z(h, Z);
        const bool has_mu = mu && h->n_cons > 0;
        if (has_mu) HIP_CHECK(hipMemcpyAsync(h->red_hmu, mu, sizeof(double) * (size_t)h->n_cons, hipMemcpyHostToDevice, h->stream));
        if (rho && h->n_cons > 0) HIP_CHECK(hipMemcpyAsync(al.hrho, rho, sizeof(double) * (size_t)h->n_cons, hipMemcpyHostToDevice, h->stream));
        if (free_mask) HIP_CHECK(hipMemcpyAsync(dmask, free_mask, bytes, hipMemcpyHostToDevice, h->stream));
        if (lo) HIP_CHECK(hipMemcpyAsync(dlo, lo, bytes, hipMemcpyHostToDevice, h->stream));
        if (hi) HIP_CHECK(hipMemcpyAsync(dhi, hi, bytes, hipMemcpyHostToDevice, h->stream));
        // the rows of the trace the step does not reach keep the caller's values
        if (trace) HIP_CHECK(hipMemcpyAsync(dtrace, trace, sizeof(double) * nt, hipMemcpyHostToDevice, h->stream));
        const NewtonBoxArgs a{free_mask ? dmask : nullptr, lo ? dlo : nullptr, hi ? dhi : nullptr, radius, shift, rtol, atol, max_iter, dp, dinfo,
                              trace ? dtrace : nullptr, entry_state ? des : nullptr, Zp ? dzp : nullptr};
        if (rho) {
            auglag_rows_at(h, al, h->d_Z, has_mu ? h->red_hmu : nullptr, al.hrho, nullptr, h->stream);
            precond_step(h, ep, h->d_Z, sigma, al.mu_eff, a, harvest, h->stream, &al);
        } else {
            precond_step(h, ep, h->d_Z, sigma, mu ? h->red_hmu : nullptr, a, harvest, h->stream);
        }
        HIP_CHECK(hipMemcpyAsync(p, dp, bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipMemcpyAsync(info, dinfo, sizeof(double) * PRECOND_INFO, hipMemcpyDeviceToHost, h->stream));
        if (trace) HIP_CHECK(hipMemcpyAsync(trace, dtrace, sizeof(double) * nt, hipMemcpyDeviceToHost, h->stream));
        if (entry_state) HIP_CHECK(hipMemcpyAsync(entry_state, des, bytes, hipMemcpyDeviceToHost, h->stream));
        if (Zp) HIP_CHECK(hipMemcpyAsync(Zp, dzp, bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_preconditioned_newton_step_dev(dto_handle* h, const double* dZ, double sigma, const double* dmu, const double* drho, const double* dfree_mask,
                                       const double* dlo, const double* dhi, double radius, double shift, double rtol, double atol,
                                       int32_t max_iter, int32_t harvest, double* dp, double* dinfo, double* dtrace, double* dentry_state,
                                       double* dZp, void* stream) {
    const std::string who = "dto_preconditioned_newton_step_dev";
    if (!h) return fail(nullptr, "null handle");
    std::string bad = newton_refusal(who, dZ, radius, shift, rtol, atol, max_iter, dp, dinfo);
    if (bad.empty()) bad = newton_box_refusal(who, (size_t)h->n_vars, dZ, dfree_mask, dlo, dhi, dp, dZp, dentry_state);
    const size_t nc = (size_t)h->n_cons, nv = (size_t)h->n_vars;
    if (bad.empty() && drho)
        bad = auglag_refusal(h, who, nullptr, {{"dp", dp, nv}, {"dZp", dZp, nv}, {"dentry_state", dentry_state, nv}, {"dinfo", dinfo, PRECOND_INFO}},
                             {{"dmu", dmu, nc}, {"drho", drho, nc}});
    if (bad.empty()) bad = precond_refusal(h, who, harvest);
    if (!bad.empty()) return fail(h, bad);
    return guarded(h, [&] {
        const ElimPlan& ep = reduced_args(h, who, true);
        reduced_workspaces(h, ep);
        precond_kernel_args(h, harvest != 0);   // before the row pass is enqueued
        block_workspaces(h, ep, 1, h->reduced_input_store && h->K >= 1);
        hipStream_t st = (hipStream_t)stream;
        const NewtonBoxArgs a{dfree_mask, dlo, dhi, radius, shift, rtol, atol, max_iter, dp, dinfo, dtrace, dentry_state, dZp};
        if (drho) {
            const AlWork A = auglag_workspaces(h, 1);
            auglag_rows_at(h, A, dZ, nc > 0 ? dmu : nullptr, drho, nullptr, st);
            precond_step(h, ep, dZ, sigma, A.mu_eff, a, harvest, st, &A);
        } else {
            precond_step(h, ep, dZ, sigma, dmu, a, harvest, st);
        }
    }, G_ASYNC, (hipStream_t)stream);
}

// z_c = P H P r_c for n_cols vectors at the store as it stands: the entry states from the mask, the preparation once, then per column
// the application's two launches -- the single application's bits
static void precondition_columns(dto_handle* h, const double* dmask, int n_cols, const double* dR, double* dZout, hipStream_t st) {
    KPrecond K = precond_kernel_args(h, false);
    K.B.mask = dmask;
    const size_t n = (size_t)h->n_vars;
    { ProfScope ps(h, st, CAT_PRECOND, (dmask ? 9.0 : 1.0) * (double)n); launch_precond_states(st, h->red, K.B); }
    precond_prepare_launches(h, K, st);
    for (int c = 0; c < n_cols; ++c) precond_apply_launches(h, K, dR + (size_t)c * n, dZout + (size_t)c * n, 0, true, st);
}
static std::string precondition_refusal(const std::string& who, size_t n, int32_t n_cols, const double* mask, const double* r, const double* z) {
    if (!r || !z) return who + ": r and z are required (NULL given)";
    if (n_cols < 1) return who + ": n_cols = " + std::to_string(n_cols) + ", at least 1 vector is required";
    if (spans_overlap(z, (size_t)n_cols * n, r, (size_t)n_cols * n)) return who + ": z overlaps r";
    if (spans_overlap(z, (size_t)n_cols * n, mask, n)) return who + ": z overlaps free_mask";
    return "";
}
int dto_newton_precondition(dto_handle* h, const double* free_mask, int32_t n_cols, const double* r, double* z) {
    const std::string who = "dto_newton_precondition";
    if (!h) return fail(nullptr, "null handle");
    const std::string bad = precondition_refusal(who, (size_t)h->n_vars, n_cols, free_mask, r, z);
    if (!bad.empty()) return fail(h, bad);
    return guarded(h, [&] {
        const ElimPlan& ep = reduced_args(h, who, false);
        reduced_workspaces(h, ep);
        const size_t n = (size_t)h->n_vars, nc = (size_t)n_cols * n;
        precond_kernel_args(h, false);
        double* q = grow_workspace(h, h->d_precond_host, n + 2 * nc);
        double *dmask = q, *dr = q + n, *dz = dr + nc;
        if (free_mask) HIP_CHECK(hipMemcpyAsync(dmask, free_mask, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(dr, r, sizeof(double) * nc, hipMemcpyHostToDevice, h->stream));
        precondition_columns(h, free_mask ? dmask : nullptr, n_cols, dr, dz, h->stream);
        HIP_CHECK(hipMemcpyAsync(z, dz, sizeof(double) * nc, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }, G_BLOCKING);
}
int dto_newton_precondition_dev(dto_handle* h, const double* dfree_mask, int32_t n_cols, const double* dr, double* dz, void* stream) {
    const std::string who = "dto_newton_precondition_dev";
    if (!h) return fail(nullptr, "null handle");
    const std::string bad = precondition_refusal(who, (size_t)h->n_vars, n_cols, dfree_mask, dr, dz);
    if (!bad.empty()) return fail(h, bad);
    return guarded(h, [&] {
        const ElimPlan& ep = reduced_args(h, who, false);
        reduced_workspaces(h, ep);
        precondition_columns(h, dfree_mask, n_cols, dr, dz, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}

// the slot a pushed pair goes to, and the store's record behind the push (the oldest pair drops at capacity)
static int pairs_push_slot(const dto_handle* h) {
    return h->pairs_count < h->newton_pairs ? precond_slot(h->pairs_head, h->pairs_count, h->newton_pairs) : h->pairs_head;
}
static void pairs_pushed(dto_handle* h) {
    if (h->pairs_count < h->newton_pairs) ++h->pairs_count;
    else h->pairs_head = (h->pairs_head + 1) % h->newton_pairs;
}
static std::string pairs_push_refusal(const dto_handle* h, const std::string& who, const double* s, const double* y, bool host) {
    if (!s || !y) return who + ": s and y are required (NULL given)";
    if (h->newton_pairs == 0)
        return who + ": the pair store has no capacity: set the option newton_pairs to 1 .. " + std::to_string(PRECOND_MAX_PAIRS) + " first (it is 0)";
    if (host)
        for (int64_t i = 0; i < h->n_vars; ++i) {
            if (!std::isfinite(s[i])) return who + ": s[" + std::to_string(i) + "] is not finite";
            if (!std::isfinite(y[i])) return who + ": y[" + std::to_string(i) + "] is not finite";
        }
    return "";
}
int dto_newton_pairs_push(dto_handle* h, const double* s, const double* y) {
    const std::string who = "dto_newton_pairs_push";
    if (!h) return fail(nullptr, "null handle");
    const std::string bad = pairs_push_refusal(h, who, s, y, true);
    if (!bad.empty()) return fail(h, bad);
    return guarded(h, [&] {
        const KPrecond K = precond_kernel_args(h, true);
        const size_t n = (size_t)h->n_vars, slot = (size_t)pairs_push_slot(h);
        HIP_CHECK(hipMemcpyAsync((double*)K.S + slot * n, s, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync((double*)K.Y + slot * n, y, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        pairs_pushed(h);
    }, G_BLOCKING);
}
int dto_newton_pairs_push_dev(dto_handle* h, const double* ds, const double* dy, void* stream) {
    const std::string who = "dto_newton_pairs_push_dev";
    if (!h) return fail(nullptr, "null handle");
    const std::string bad = pairs_push_refusal(h, who, ds, dy, false);
    if (!bad.empty()) return fail(h, bad);
    return guarded(h, [&] {
        const KPrecond K = precond_kernel_args(h, true);
        const size_t n = (size_t)h->n_vars, slot = (size_t)pairs_push_slot(h);
        hipStream_t st = (hipStream_t)stream;
        { ProfScope ps(h, st, CAT_PRECOND, 16.0 * (double)n); launch_precond_copy(st, (int64_t)n, ds, (double*)K.S + slot * n); }
        { ProfScope ps(h, st, CAT_PRECOND, 16.0 * (double)n); launch_precond_copy(st, (int64_t)n, dy, (double*)K.Y + slot * n); }
        pairs_pushed(h);
    }, G_ASYNC, (hipStream_t)stream);
}
int dto_newton_pairs_clear(dto_handle* h) {
    if (!h) return fail(nullptr, "null handle");
    h->pairs_count = h->pairs_head = 0;
    return 0;
}
int dto_newton_pairs_info(dto_handle* h, int32_t* count, int32_t* capacity) {
    if (!h) return fail(nullptr, "null handle");
    if (count) *count = h->pairs_count;
    if (capacity) *capacity = h->newton_pairs;
    return 0;
}

// ---- reduced-space minimize (include/dto_engine.h, "Reduced-space minimize"; dto_minimize.hip, dto_minimize_plan.h): minimize_solve's
// loop with the step, the merit and the row pass above as its three callables, all unchanged, and one small launch behind every trial
// and every outer iteration.

// what the device routine takes: device pointers, Z / mu / rho in and out
struct MinimizeArgs {
    double *Z, *mu, *rho;
    const double *mask, *lo, *hi;
    MinimizeOptions opt;
    int outer, trials, harvest;
    double *info, *history, *outer_history, *entry_state;
};

// d_minimize's parts
struct MinWork { double *p, *Zp, *Zt, *sinfo, *bank, *rinfo0, *rinfo, *phi_t, *mail; };

static MinWork minimize_workspaces(dto_handle* h) {
    const size_t n = (size_t)h->n_vars;
    double* q = grow_workspace(h, h->d_minimize, 3 * n + MINIMIZE_STEP_INFO + 2 * MINIMIZE_STATE + 2 * AL_INFO + 4 + MINIMIZE_MAIL);
    MinWork M{};
    M.p = q; M.Zp = q + n; M.Zt = q + 2 * n; M.sinfo = q + 3 * n;
    M.bank = M.sinfo + MINIMIZE_STEP_INFO; M.rinfo0 = M.bank + 2 * MINIMIZE_STATE; M.rinfo = M.rinfo0 + AL_INFO;
    M.phi_t = M.rinfo + AL_INFO; M.mail = M.phi_t + 4;
    return M;
}

// The device routine both entry-point families run: everything on `st`, every pointer a device pointer.
static void minimize_run(dto_handle* h, const ElimPlan& ep, const FeasiblePlan& fp, double sigma, const MinimizeArgs& a, hipStream_t st) {
    const bool pre = h->newton_pairs > 0, has_rho = a.rho != nullptr;
    const bool store_route = h->reduced_input_store && h->K >= 1;
    const double* opt = a.opt.v;
    // every workspace before anything is enqueued
    const MinWork M = minimize_workspaces(h);
    const FeasWork W = feasible_workspaces(h, fp, true);
    block_workspaces(h, ep, 1, store_route);
    if (pre) precond_kernel_args(h, a.harvest != 0);
    else grow_workspace(h, h->d_newton_box, (size_t)newton_box_workspace_doubles(h->n_vars));
    AlWork al{};
    if (has_rho) al = auglag_workspaces(h, 1);
    const double* mu = h->n_cons > 0 ? a.mu : nullptr;
    const int outer = has_rho ? a.outer : 1;

    auto merit = [&](const double* Zin, double* Zout, double* dphi) {   // dto_auglag_merit_dev's launches
        if (!has_rho) {
            feasible_merit(h, fp, W, Zin, sigma, mu, dphi, Zout, nullptr, st);
            return;
        }
        feasible_trajectory(h, fp, Zin, Zout, st);
        do_objective(h, Zout, W.f, st);
        do_constraint(h, Zout, W.g, st);
        auglag_row_pass(h, W.g, mu, a.rho, nullptr, nullptr, al.info, sigma, W.f, dphi, st);
    };
    auto step = [&](double delta) {   // dto_preconditioned_newton_step_dev's launches, or dto_auglag_newton_step_dev's
        const NewtonBoxArgs b{a.mask, a.lo, a.hi, delta, opt[MIN_OPT_SHIFT], opt[MIN_OPT_RTOL], opt[MIN_OPT_ATOL], (int)opt[MIN_OPT_MAX_ITER],
                              M.p, M.sinfo, nullptr, a.entry_state, M.Zp};
        const double* m = mu;
        if (has_rho) {
            auglag_rows_at(h, al, a.Z, mu, a.rho, nullptr, st);
            m = al.mu_eff;
        }
        if (pre) precond_step(h, ep, a.Z, sigma, m, b, a.harvest, st, has_rho ? &al : nullptr);
        else newton_box_step(h, ep, a.Z, sigma, m, b, st, has_rho ? &al : nullptr);
    };
    auto mail = [&] {   // the one readback behind a launch of dto_minimize.hip
        HIP_CHECK(hipMemcpyAsync(h->mailbox->minimize, M.mail, MINIMIZE_MAIL * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return h->mailbox->minimize;
    };

    KMinimize K{};
    K.n = h->n_vars; K.n_dyn = h->n_dyn; K.n_cons = h->n_cons;
    K.Z = a.Z; K.Zt = M.Zt; K.sinfo = M.sinfo; K.phi_t = M.phi_t; K.rinfo = M.rinfo; K.rinfo0 = M.rinfo0;
    K.mu = a.mu; K.rho = a.rho; K.mu_eff = al.mu_eff; K.mail = M.mail; K.info = a.info; K.opt = a.opt;
    int q = 0;   // launches of dto_minimize.hip so far: bank q % 2 is current
    auto banks = [&] {
        K.bank_in = M.bank + MINIMIZE_STATE * (q % 2);
        K.bank_out = M.bank + MINIMIZE_STATE * ((q + 1) % 2);
    };
    const double scalars = 8.0 * (2.0 * MINIMIZE_STATE + MINIMIZE_INFO + MINIMIZE_HISTORY + MINIMIZE_MAIL + 5.0);
    HIP_CHECK(hipMemsetAsync(M.bank, 0, 2 * MINIMIZE_STATE * sizeof(double), st));
    if (has_rho) auglag_rows_at(h, al, a.Z, mu, a.rho, M.rinfo0, st);   // the first max viol
    int64_t trial = 0;
    for (int o = 0; o < outer; ++o) {
        merit(a.Z, a.Z, M.bank + MINIMIZE_STATE * (q % 2) + MNS_PHI);   // Z becomes its feasible trajectory
        double delta = opt[MIN_OPT_RADIUS0];
        int stop = MIN_STOP_NONE;
        for (int t = 0; t < a.trials && stop == MIN_STOP_NONE; ++t, ++trial) {
            step(delta);
            // the gradient test stands in front of the merit, so the host reads the step's ||g|| (the step has just waited for its own
            // status: the stream is idle)
            HIP_CHECK(hipMemcpyAsync(h->mailbox->minimize_step, M.sinfo, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            const bool gradient = h->mailbox->minimize_step[2] <= opt[MIN_OPT_GTOL];
            if (!gradient) merit(M.Zp, M.Zt, M.phi_t);
            banks();
            K.row = a.history ? a.history + MINIMIZE_HISTORY * trial : nullptr;
            K.F = MinimizeTrialFlags{q == 0, t == 0, t == a.trials - 1, gradient, has_rho, pre ? 16 : 12};
            {   // bytes as if the trial is accepted: Zt read and Z written, and the scalars
                ProfScope ps(h, st, CAT_MINIMIZE, (gradient ? 0.0 : 16.0 * (double)h->n_vars) + scalars);
                launch_minimize_trial(st, K);
            }
            ++q;
            const double* m = mail();
            delta = m[MNM_DELTA];
            stop = (int)m[MNM_STOP];
        }
        if (stop == MIN_STOP_NOT_FINITE || !has_rho) break;
        auglag_rows_at(h, al, a.Z, mu, a.rho, M.rinfo, st);
        banks();
        K.row = a.outer_history ? a.outer_history + MINIMIZE_OUTER_HISTORY * o : nullptr;
        K.first_outer = o == 0; K.last_outer = o == outer - 1;
        {
            ProfScope ps(h, st, CAT_MINIMIZE, 32.0 * (double)(h->n_cons - h->n_dyn) + scalars + 8.0 * 2.0 * AL_INFO);
            launch_minimize_outer(st, K);
        }
        ++q;
        if (mail()[MNM_STOP] != 0.0) break;
    }
}

static std::string minimize_refusal(const dto_handle* h, const std::string& who, const double* Z, const double* mu, const double* rho,
                                    const double* rho_host, const double* mask, const double* lo, const double* hi, const double* options,
                                    int32_t outer, int32_t trials, int32_t harvest, const double* info, const double* history,
                                    const double* outer_history, const double* entry_state, MinimizeOptions* out) {
    static const char* names[MINIMIZE_OPTIONS] = {"radius0", "eta_accept", "eta_shrink", "eta_grow", "shrink_div", "grow_mul", "radius_max", "radius_min",
                                                  "gtol", "ctol", "viol_div", "rho_mul", "shift", "rtol", "atol", "max_iter"};
    if (!Z || !info) return who + ": Z and info are required (NULL given)";
    if (outer < 1) return who + ": outer = " + std::to_string(outer) + ", at least 1 outer iteration is required";
    if (trials < 1) return who + ": trials = " + std::to_string(trials) + ", at least 1 trial is required";
    if (!rho && outer != 1) return who + ": outer = " + std::to_string(outer) + " without rho: without penalties there is one outer iteration";
    if (rho && !mu) return who + ": rho is given and mu is NULL: the multipliers are an output of the outer loop";
    MinimizeOptions O = minimize_default_options();
    if (options)
        for (int i = 0; i < MINIMIZE_OPTIONS; ++i) O.v[i] = options[i];
    const double* v = O.v;
    for (int i = 0; i < MINIMIZE_OPTIONS; ++i)
        if (!(v[i] >= 0.0)) return who + ": option " + names[i] + " = " + std::to_string(v[i]) + " is negative or a NaN";
    if (!(v[MIN_OPT_RADIUS0] > 0.0) || !std::isfinite(v[MIN_OPT_RADIUS0])) return who + ": option radius0 must be finite and > 0";
    if (!(v[MIN_OPT_ETA_ACCEPT] <= v[MIN_OPT_ETA_SHRINK] && v[MIN_OPT_ETA_SHRINK] < v[MIN_OPT_ETA_GROW]))
        return who + ": the options must satisfy 0 <= eta_accept <= eta_shrink < eta_grow";
    if (!(v[MIN_OPT_SHRINK_DIV] > 1.0)) return who + ": option shrink_div must be > 1";
    if (!(v[MIN_OPT_GROW_MUL] >= 1.0)) return who + ": option grow_mul must be >= 1";
    if (!(v[MIN_OPT_MAX_ITER] <= 2147483647.0) || v[MIN_OPT_MAX_ITER] != std::floor(v[MIN_OPT_MAX_ITER]))
        return who + ": option max_iter must be a whole number";
    std::string bad = newton_refusal(who, Z, v[MIN_OPT_RADIUS0], v[MIN_OPT_SHIFT], v[MIN_OPT_RTOL], v[MIN_OPT_ATOL], (int32_t)v[MIN_OPT_MAX_ITER], Z, info);
    if (!bad.empty()) return bad;
    const size_t nv = (size_t)h->n_vars, nc = (size_t)h->n_cons, nh = MINIMIZE_HISTORY * (size_t)outer * (size_t)trials;
    if (rho) {
        bad = auglag_refusal(h, who, rho_host, {}, {});
        if (!bad.empty()) return bad;
    }
    bad = precond_refusal(h, who, harvest);
    if (!bad.empty()) return bad;
    const AlSpan outs[] = {{"Z", Z, nv}, {"mu", rho ? mu : nullptr, nc}, {"rho", rho, nc}, {"info", info, MINIMIZE_INFO}, {"history", history, nh},
                           {"outer_history", outer_history, MINIMIZE_OUTER_HISTORY * (size_t)outer}, {"entry_state", entry_state, nv}};
    const AlSpan ins[] = {{"mu", rho ? nullptr : mu, nc}, {"free_mask", mask, nv}, {"lo", lo, nv}, {"hi", hi, nv}};
    for (size_t i = 0; i < sizeof(outs) / sizeof(outs[0]); ++i) {
        for (const AlSpan& in : ins)
            if (spans_overlap(outs[i].p, outs[i].n, in.p, in.n)) return who + ": " + outs[i].name + " overlaps " + in.name;
        for (size_t j = i + 1; j < sizeof(outs) / sizeof(outs[0]); ++j)
            if (spans_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n)) return who + ": " + outs[i].name + " overlaps " + outs[j].name;
    }
    *out = O;
    return "";
}

int dto_projected_minimize_dev(dto_handle* h, double* dZ, double sigma, double* dmu, double* drho, const double* dfree_mask, const double* dlo,
                             const double* dhi, const double* options, int32_t outer, int32_t trials, int32_t harvest, double* dinfo,
                             double* dhistory, double* douter_history, double* dentry_state, void* stream) {
    const std::string who = "dto_projected_minimize_dev";
    if (!h) return fail(nullptr, "null handle");
    MinimizeOptions O{};
    const std::string bad = minimize_refusal(h, who, dZ, dmu, drho, nullptr, dfree_mask, dlo, dhi, options, outer, trials, harvest, dinfo, dhistory,
                                             douter_history, dentry_state, &O);
    if (!bad.empty()) return fail(h, bad);
    return guarded(h, [&] {
        const ElimPlan& ep = reduced_args(h, who, true);
        const FeasiblePlan& fp = feasible_args(h, who, true);
        reduced_workspaces(h, ep);
        const MinimizeArgs a{dZ, dmu, drho, dfree_mask, dlo, dhi, O, outer, trials, harvest, dinfo, dhistory, douter_history, dentry_state};
        minimize_run(h, ep, fp, sigma, a, (hipStream_t)stream);
    }, G_ASYNC, (hipStream_t)stream);
}

int dto_projected_minimize(dto_handle* h, double* Z, double sigma, double* mu, double* rho, const double* free_mask, const double* lo,
                         const double* hi, const double* options, int32_t outer, int32_t trials, int32_t harvest, double* info, double* history,
                         double* outer_history, double* entry_state) {
    const std::string who = "dto_projected_minimize";
    if (!h) return fail(nullptr, "null handle");
    MinimizeOptions O{};
    const std::string bad = minimize_refusal(h, who, Z, mu, rho, rho, free_mask, lo, hi, options, outer, trials, harvest, info, history,
                                             outer_history, entry_state, &O);
    if (!bad.empty()) return fail(h, bad);
    return guarded(h, [&] {
        const ElimPlan& ep = reduced_args(h, who, true);
        const FeasiblePlan& fp = feasible_args(h, who, true);
        reduced_workspaces(h, ep);
        const size_t n = (size_t)h->n_vars, nc = (size_t)std::max<int64_t>(h->n_cons, 1), bytes = sizeof(double) * n;
        const size_t nh = MINIMIZE_HISTORY * (size_t)outer * (size_t)trials, no = MINIMIZE_OUTER_HISTORY * (size_t)outer;
        // every workspace before the uploads are enqueued
        minimize_workspaces(h);
        feasible_workspaces(h, fp, true);
        block_workspaces(h, ep, 1, h->reduced_input_store && h->K >= 1);
        if (h->newton_pairs > 0) precond_kernel_args(h, harvest != 0);
        else grow_workspace(h, h->d_newton_box, (size_t)newton_box_workspace_doubles(h->n_vars));
        if (rho) auglag_workspaces(h, 1);
        double* q = grow_workspace(h, h->d_minimize_host, 5 * n + 2 * nc + MINIMIZE_INFO + nh + no);
        double *dZ = q, *dmask = q + n, *dlo = q + 2 * n, *dhi = q + 3 * n, *des = q + 4 * n, *dmu = q + 5 * n, *drho = dmu + nc;
        double *dinfo = drho + nc, *dhist = dinfo + MINIMIZE_INFO, *dohist = dhist + nh;
        hipStream_t st = h->stream;
        const bool has_mu = mu && h->n_cons > 0, has_rho = rho != nullptr;
        HIP_CHECK(hipMemcpyAsync(dZ, Z, bytes, hipMemcpyHostToDevice, st));
        if (has_mu) HIP_CHECK(hipMemcpyAsync(dmu, mu, sizeof(double) * nc, hipMemcpyHostToDevice, st));
        if (has_rho && h->n_cons > 0) HIP_CHECK(hipMemcpyAsync(drho, rho, sizeof(double) * nc, hipMemcpyHostToDevice, st));
        if (free_mask) HIP_CHECK(hipMemcpyAsync(dmask, free_mask, bytes, hipMemcpyHostToDevice, st));
        if (lo) HIP_CHECK(hipMemcpyAsync(dlo, lo, bytes, hipMemcpyHostToDevice, st));
        if (hi) HIP_CHECK(hipMemcpyAsync(dhi, hi, bytes, hipMemcpyHostToDevice, st));
        // the rows of the histories the loop does not reach keep the caller's values
        if (history) HIP_CHECK(hipMemcpyAsync(dhist, history, sizeof(double) * nh, hipMemcpyHostToDevice, st));
        if (outer_history) HIP_CHECK(hipMemcpyAsync(dohist, outer_history, sizeof(double) * no, hipMemcpyHostToDevice, st));
        if (entry_state) HIP_CHECK(hipMemcpyAsync(des, entry_state, bytes, hipMemcpyHostToDevice, st));
        const MinimizeArgs a{dZ, has_mu ? dmu : nullptr, has_rho ? drho : nullptr, free_mask ? dmask : nullptr, lo ? dlo : nullptr, hi ? dhi : nullptr,
                             O, outer, trials, harvest, dinfo, history ? dhist : nullptr, outer_history ? dohist : nullptr,
                             entry_state ? des : nullptr};
        minimize_run(h, ep, fp, sigma, a, st);
        HIP_CHECK(hipMemcpyAsync(Z, dZ, bytes, hipMemcpyDeviceToHost, st));
        if (has_rho && h->n_cons > 0) {
            HIP_CHECK(hipMemcpyAsync(mu, dmu, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(rho, drho, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipMemcpyAsync(info, dinfo, sizeof(double) * MINIMIZE_INFO, hipMemcpyDeviceToHost, st));
        if (history) HIP_CHECK(hipMemcpyAsync(history, dhist, sizeof(double) * nh, hipMemcpyDeviceToHost, st));
        if (outer_history) HIP_CHECK(hipMemcpyAsync(outer_history, dohist, sizeof(double) * no, hipMemcpyDeviceToHost, st));
        if (entry_state) HIP_CHECK(hipMemcpyAsync(entry_state, des, bytes, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }, G_BLOCKING);
}

// ---- multi-GPU: ranges, gather plans, collectives (dto_comm.h)
int dto_comm_unique_id(void* id128) {
    if (!id128) return fail(nullptr, "dto_comm_unique_id: null argument");
    const std::string e = Comm::unique_id(id128);
    return e.empty() ? 0 : fail(nullptr, e);
}

int dto_comm_create(dto_handle* h, const void* id128, int32_t rank, int32_t world) {
    return comm_guarded(h, [&] {
        if (!id128) throw HipError{"dto_comm_create: null id"};
        if (h->comm) throw HipError{"dto_comm_create: the handle already has a communicator (dto_comm_destroy first)"};
        std::string err;
        std::unique_ptr<Comm> c = Comm::create(id128, rank, world, err);
        if (!c) throw HipError{err};
        // every rank's knot range: one 16-byte all-gather
        if (!h->d_ranges) h->d_ranges = own(h, dalloc<int64_t>(2 * 1024));
        if (world > 1023) throw HipError{"dto_comm_create: at most 1023 ranks"};
        const int64_t mine[2] = {h->k_lo, h->k_hi};
        HIP_CHECK(hipMemcpyAsync(h->d_ranges, mine, sizeof(mine), hipMemcpyHostToDevice, h->stream));
        err = c->all_gather_i64(h->d_ranges, h->d_ranges + 2, 2, h->stream);
        if (!err.empty()) throw HipError{err};
        std::vector<int64_t> all((size_t)2 * world);
        HIP_CHECK(hipMemcpyAsync(all.data(), h->d_ranges + 2, sizeof(int64_t) * all.size(), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        std::vector<int64_t> lo(world), hi(world);
        for (int r = 0; r < world; ++r) { lo[r] = all[2 * r]; hi[r] = all[2 * r + 1]; }
        set_ranges(h, rank, world, lo.data(), hi.data());
        h->comm = std::move(c);
    });
}

int dto_comm_set_ranges(dto_handle* h, int32_t rank, int32_t world, const int64_t* k_lo, const int64_t* k_hi) {
    return comm_guarded(h, [&] {
        if (!k_lo || !k_hi) throw HipError{"dto_comm_set_ranges: null argument"};
        if (h->comm) throw HipError{"dto_comm_set_ranges: the handle's communicator already fixed the ranges"};
        set_ranges(h, rank, world, k_lo, k_hi);
    }, /*needs_device=*/false);
}

int dto_comm_destroy(dto_handle* h) {
    return comm_guarded(h, [&] {
        h->comm.reset();
        h->rank_ranges.clear();
        h->comm_rank = -1;
    }, /*needs_device=*/!(h && h->structure_only));
}

int dto_get_gather_layout(const dto_handle* h, int32_t vector, dto_gather_layout* out) {
    dto_handle* hm = const_cast<dto_handle*>(h);
    return comm_guarded(hm, [&] {
        if (!out) throw HipError{"dto_get_gather_layout: null argument"};
        dto_gather_layout L{};
        L.world = (int32_t)h->rank_ranges.size();
        if (vector == DTO_VECTOR_CONSTRAINT) {
            if (h->rank_ranges.empty()) throw HipError{"no knot ranges yet: dto_comm_create / dto_comm_set_ranges first"};
            L.total = L.padded_len = h->n_cons;
            L.own_len = h->cons_len;
        } else {
            const GatherPlan& pl = plan_of(h, vector);
            L.total = pl.total;
            L.padded_len = pl.padded_len();
            L.front_pad = pl.in_place ? pl.front : 0;
            L.own_lo = pl.slabs[h->comm_rank].lo;
            L.own_len = pl.slabs[h->comm_rank].len;
            L.in_place_all_gather = pl.in_place ? 1 : 0;
        }
        *out = L;
    }, /*needs_device=*/false);
}

int dto_gather_slabs(const dto_handle* h, int32_t vector, int64_t* lo, int64_t* len) {
    dto_handle* hm = const_cast<dto_handle*>(h);
    return comm_guarded(hm, [&] {
        if (!lo || !len) throw HipError{"dto_gather_slabs: null argument"};
        const GatherPlan& pl = plan_of(h, vector);
        for (size_t r = 0; r < pl.slabs.size(); ++r) { lo[r] = pl.slabs[r].lo; len[r] = pl.slabs[r].len; }
    }, /*needs_device=*/false);
}

int dto_gather_jacobian_dev(dto_handle* h, double* dbuf, void* stream) {
    return comm_guarded(h, [&] { gather_vector(h, DTO_VECTOR_JACOBIAN, dbuf, (hipStream_t)stream); });
}
int dto_gather_hessian_dev(dto_handle* h, double* dbuf, void* stream) {
    return comm_guarded(h, [&] { gather_vector(h, DTO_VECTOR_HESSIAN, dbuf, (hipStream_t)stream); });
}
int dto_gather_gradient_dev(dto_handle* h, double* dbuf, void* stream) {
    return comm_guarded(h, [&] { gather_vector(h, DTO_VECTOR_GRADIENT, dbuf, (hipStream_t)stream); });
}
int dto_gather_constraint_dev(dto_handle* h, const double* dg_local, double* dg_full, void* stream) {
    return comm_guarded(h, [&] {
        if (!h->comm) throw HipError{"dto_gather: no communicator (dto_comm_create)"};
        hipStream_t st = (hipStream_t)stream;
        int64_t at = 0;
        for (auto& sg : h->row_segments) {  // the local buffer is the concatenation of the rank's segments
            HIP_CHECK(hipMemcpyAsync(dg_full + sg.first, dg_local + at, sizeof(double) * (size_t)sg.second, hipMemcpyDeviceToDevice, st));
            at += sg.second;
        }
        const std::string e = h->comm->broadcast_slabs(dg_full, h->cons_segments, h->cons_segment_root, st);
        if (!e.empty()) throw HipError{e};
    });
}
int dto_allreduce_objective_dev(dto_handle* h, double* df, void* stream) {
    return comm_guarded(h, [&] {
        if (!h->comm) throw HipError{"dto_allreduce_objective_dev: no communicator (dto_comm_create)"};
        const std::string e = h->comm->all_reduce_sum(df, 1, (hipStream_t)stream);
        if (!e.empty()) throw HipError{e};
    });
}

int dto_bind_output_dev(dto_handle* h, int32_t vector, double* dptr) {
    if (!h) return fail(nullptr, "null handle");
    if (vector != DTO_VECTOR_JACOBIAN && vector != DTO_VECTOR_HESSIAN) return fail(h, "dto_bind_output_dev: the Jacobian or the Hessian value vector");
    const int w = vector == DTO_VECTOR_JACOBIAN ? 0 : 1;
    h->bound[w] = dptr;
    h->primed[w] = false;
    return 0;
}

// ---- measurement
int dto_set_option(dto_handle* h, const char* name, int64_t value) {
    if (!h || !name) return 1;
    ++h->gen;  // any option may change what the Hessian-vector products' cached point holds
    if (std::string(name) == "reuse_forward_sweep") {
        h->reuse = value != 0;
        drop_caches(h);
        return 0;
    }
    if (std::string(name) == "overlap_sweep") {
        h->overlap_sweep = value != 0;
        return 0;
    }
    if (std::string(name) == "chain_form") {
        if (value != 0 && value != 1) return fail(h, "dto_set_option: chain_form takes 0 (one launch per call for 33..64 states) or 1 (batched-GEMM launches)");
        h->chain_form = (int)value;
        return 0;
    }
    if (std::string(name) == "sweep_form") {
        if (value != 0 && value != 1) return fail(h, "dto_set_option: sweep_form takes 0 (fused where it applies) or 1 (step per launch)");
        h->sweep_form = (int)value;
        drop_caches(h);
        return 0;
    }
    if (std::string(name) == "host_xfer") {
        if (h->plans_built) return fail(h, "dto_set_option: host_xfer must be set before the first host-pointer Jacobian / Hessian call");
        h->host_xfer = value != 0;
        return 0;
    }
    if (std::string(name) == "chain_chunk") {
        if (value < 0) return fail(h, "dto_set_option: chain_chunk must be >= 0");
        h->chain_chunk = (int)std::min<int64_t>(value, 1 << 30);
        return 0;
    }
    if (std::string(name) == "debug_bad_launch") {
#ifdef DTO_TUNING
        h->P.debug_bad_launch = value != 0;
        return 0;
#else
        return fail(h, "dto_set_option: debug_bad_launch exists in TUNING builds only (make TUNING=1: libdto_engine_t.so)");
#endif
    }
    if (std::string(name) == "host_xfer_check") {
        h->xfer_check = value != 0;
        return 0;
    }
    if (std::string(name) == "deterministic") {
        h->deterministic = value != 0;
        drop_caches(h);
        return 0;
    }
    if (std::string(name) == "tdb_matrix_free_products") {
        if (value != 0 && value != 1)
            return fail(h, "dto_set_option: tdb_matrix_free_products takes 0 (J w / J' w of time-dependent integrators through the value slab) or 1 (matrix-free)");
        h->tdb_matrix_free_products = (int)value;
        return 0;
    }
    if (std::string(name) == "newton_pairs") {
        if (value < 0 || value > PRECOND_MAX_PAIRS)
            return fail(h, "dto_set_option: newton_pairs takes 0 (no preconditioner) .. " + std::to_string(PRECOND_MAX_PAIRS) +
                               ", the most pairs dto_preconditioned_newton_step keeps");
        h->newton_pairs = (int)value;
        h->pairs_bank = h->pairs_count = h->pairs_head = 0;   // setting the option clears the store
        return 0;
    }
    if (std::string(name) == "reduced_input_store") {
        if (value != 0 && value != 1)
            return fail(h, "dto_set_option: reduced_input_store takes 0 (J v^ and J' w of the reduced-space operators through dto_eval_jacobian_product / _transpose_product) or 1 (from the kept input blocks)");
        h->reduced_input_store = (int)value;
        return 0;
    }
    if (std::string(name) == "reduced_block_width") {
        if (value < 0 || value > 64)
            return fail(h, "dto_set_option: reduced_block_width takes 0 (the engine's choice) or 1 .. 64, the most columns per chunk of dto_eval_hessian_products / dto_projected_hessian_products");
        h->reduced_block_width = (int)value;
        return 0;
    }
    if (std::string(name) == "tdb_share_members") {
        int cap = 1;
        for (const TdbHost& t : h->tdb) cap = std::max(cap, t.share_active ? t.share_cap : 1);
        if (value < 1 || value > cap)
            return fail(h, "dto_set_option: tdb_share_members takes 1 (one launch per member) .. " + std::to_string(cap) +
                               ", the largest group launch this handle was created for");
        h->tdb_share_members = (int)value;
        return 0;
    }
    if (std::string(name) == "tdb_resident") {
        int most = 0;
        for (const TdbHost& t : h->tdb)
            if (t.mfma || t.kron) most = std::max(most, t.resident);
        if (value < 0 || value > most)
            return fail(h, "dto_set_option: tdb_resident takes 0 (the default grid) .. " + std::to_string(most) +
                               ", the largest persistent grid of this handle's k_tdb_mfma / k_tdb_kron integrators");
        h->tdb_resident = (int)value;
        return 0;
    }
    if (std::string(name) == "expm_form") {
        if (value != 0 && value != 2 && value != 3) return fail(h, "dto_set_option: expm_form takes 0 (by cost), 2 or 3");
        h->expm_form = (int)value;
        return 0;
    }
    return fail(h, std::string("dto_set_option: unknown option ") + name);
}

int dto_profile_enable(dto_handle* h, int32_t on) {
    if (!h) return 1;
    if (on && !h->structure_only && h->ev_pool.size() < 1024) {
        (void)hipSetDevice(h->device);
        while (h->ev_pool.size() < 1024) {  // enough for ~8 calls without touching the allocator in the timed region
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) break;
            h->ev_pool.push_back(e);
        }
    }
    h->profiling = on != 0;
    return 0;
}
int dto_profile_reset(dto_handle* h) {
    if (!h) return 1;
    for (auto& r : h->prof) { h->ev_pool.push_back(r.a); h->ev_pool.push_back(r.b); }
    h->prof.clear();
    for (auto& c : h->sweep_forms) c = 0;
    return 0;
}
int dto_profile_get(dto_handle* h, const char* name, double* ms, int64_t* launches, double* flops) {
    return guarded(h, [&] {
        int cat = -1;
        bool any_gemm = false, any_basis = false, any_rollout = false, any_dynsolve = false;
        if (!strcmp(name, "bgemm")) any_gemm = true;
        else if (!strcmp(name, "bgemm_horner")) cat = CAT_BGEMM_HORNER;
        else if (!strcmp(name, "bgemm_square")) cat = CAT_BGEMM_SQUARE;
        else if (!strcmp(name, "bgemm_plain")) cat = CAT_BGEMM;
        else if (!strcmp(name, "chain64")) cat = CAT_CHAIN64;
        else if (!strcmp(name, "basis")) any_basis = true;
        else if (!strcmp(name, "basis_k")) cat = CAT_OTHER;
        else if (!strcmp(name, "basis_multi")) cat = CAT_BASIS_MULTI;
        else if (!strcmp(name, "zero_fill")) cat = CAT_ZERO;
        else if (!strcmp(name, "build_A")) cat = CAT_BUILD_A;
        else if (!strcmp(name, "assembly")) cat = CAT_ASSEMBLY;
        else if (!strcmp(name, "expmv")) cat = CAT_SWEEP;
        else if (!strcmp(name, "expmv_adjoint")) cat = CAT_SWEEP_ADJOINT;
        else if (!strcmp(name, "hess_product")) cat = CAT_HESS_PRODUCT;
        else if (!strcmp(name, "share")) cat = CAT_SHARE;
        else if (!strcmp(name, "tdb_mfma")) cat = CAT_TDB_MFMA;
        else if (!strcmp(name, "tdb_kron")) cat = CAT_TDB_KRON;
        else if (!strcmp(name, "jac_product")) cat = CAT_JAC_PRODUCT;
        else if (!strcmp(name, "tdb_product")) cat = CAT_TDB_PRODUCT;
        else if (!strcmp(name, "rollout")) any_rollout = true;
        else if (!strcmp(name, "rollout_gather")) cat = CAT_ROLLOUT;
        else if (!strcmp(name, "rollout_tree")) cat = CAT_ROLLOUT_TREE;
        else if (!strcmp(name, "rollout_descent")) cat = CAT_ROLLOUT_DESCENT;
        else if (!strcmp(name, "dynsolve")) any_dynsolve = true;
        else if (!strcmp(name, "dynsolve_tree")) cat = CAT_DYNSOLVE_TREE;
        else if (!strcmp(name, "dynsolve_scan")) cat = CAT_DYNSOLVE_SCAN;
        else if (!strcmp(name, "dynsolve_couple")) cat = CAT_DYNSOLVE_COUPLE;
        else if (!strcmp(name, "dynsolve_deriv")) cat = CAT_DYNSOLVE_DERIV;
        else if (!strcmp(name, "reduced_pack")) cat = CAT_REDUCED_PACK;
        else if (!strcmp(name, "reduced_input")) cat = CAT_REDUCED_INPUT;
        else if (!strcmp(name, "feasible")) cat = CAT_FEASIBLE;
        else if (!strcmp(name, "newton")) cat = CAT_NEWTON;
        else if (!strcmp(name, "newton_box")) cat = CAT_NEWTON_BOX;
        else if (!strcmp(name, "auglag")) cat = CAT_AUGLAG;
        else if (!strcmp(name, "precond")) cat = CAT_PRECOND;
        else if (!strcmp(name, "minimize")) cat = CAT_MINIMIZE;
        else if (!strcmp(name, "hess_product_setup")) {
            // host time of the products' index build (once per handle), no launches; third output: device bytes of the private
            // slab and the index
            if (ms) *ms = h->hp_setup_ms;
            if (launches) *launches = 0;
            if (flops) *flops = h->hp_bytes;
            return;
        }
        else if (!strncmp(name, "sweep_", 6)) {
            // generator sweeps by the form they took (run_sweep): a count, no timing, no flops; they feed no other name
            static const char* const forms[5] = {"sweep_gs", "sweep_fused", "sweep_s64", "sweep_cluster", "sweep_step"};
            int f = 0;
            while (f < 5 && strcmp(name, forms[f])) ++f;
            if (f == 5) throw HipError{"dto_profile_get: unknown name"};
            if (ms) *ms = 0.0;
            if (launches) *launches = h->sweep_forms[f];
            if (flops) *flops = 0.0;
            return;
        }
        else if (strcmp(name, "all")) throw HipError{"dto_profile_get: unknown name"};
        double tot = 0, fl = 0;
        int64_t n = 0;
        for (auto& r : h->prof) {
            if (any_gemm && r.cat != CAT_BGEMM && r.cat != CAT_BGEMM_HORNER && r.cat != CAT_BGEMM_SQUARE && r.cat != CAT_CHAIN64) continue;
            if (any_basis && r.cat != CAT_OTHER && r.cat != CAT_BASIS_MULTI) continue;
            if (!any_gemm && !any_basis && cat >= 0 && r.cat != cat) continue;
            if (is_rollout_cat(r.cat) ? !(any_rollout || r.cat == cat) : any_rollout) continue;   // ("all": the rollout is no callback)
            if (is_dynsolve_cat(r.cat) ? !(any_dynsolve || r.cat == cat) : any_dynsolve) continue;   // (nor are the solves)
            if (is_elim_cat(r.cat) && r.cat != cat) continue;
            if ((r.cat == CAT_REDUCED_PACK || r.cat == CAT_REDUCED_INPUT || r.cat == CAT_FEASIBLE || r.cat == CAT_NEWTON || r.cat == CAT_NEWTON_BOX ||
                 r.cat == CAT_AUGLAG || r.cat == CAT_PRECOND || r.cat == CAT_MINIMIZE) && r.cat != cat) continue;
            HIP_CHECK(hipEventSynchronize(r.b));
            float t = 0;
            HIP_CHECK(hipEventElapsedTime(&t, r.a, r.b));
            tot += t; ++n;
            if (cat == CAT_SHARE || r.cat != CAT_SHARE) fl += r.flops;  // (priced in bytes: not part of the sum of "all")
        }
        if (ms) *ms = tot;
        if (launches) *launches = n;
        if (flops) *flops = fl;
    });
}
int dto_last_stats(const dto_handle* h, int32_t* max_squarings, int32_t* expmv_terms) {
    if (!h) return 1;
    dto_handle* hm = const_cast<dto_handle*>(h);
    // the deferred error of an asynchronous call surfaces here (guarded looks at the pending statistics first); the
    // statistics themselves are then read again so that `expmv_terms` is current after blocking calls as well
    int rc = guarded(hm, [&] { HIP_CHECK(hipDeviceSynchronize()); }, G_BLOCKING);
    if (max_squarings) *max_squarings = h->last_smax;
    if (expmv_terms) *expmv_terms = h->last_terms;
    return rc;
}

}  // extern "C"
