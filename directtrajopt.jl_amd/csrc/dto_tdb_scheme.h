// dto_tdb_scheme.h -- the discrete scheme of the device TimeDependentBilinearIntegrator: parameter and table counts, the ranking of
// the upper-triangle parameter pairs, and the classical RK4 tableau forward and as the discrete adjoint.  Plain C++ (no HIP header,
// no engine header): the same functions run in the kernels, in the host's checks and in a g++-built test.
// Who uses what: the counts and the table check serve the host code of all three kernels (dto_tdb.hip, dto_tdb_mfma.hip,
// dto_tdb_kron.hip) and the layouts of the latter two; the pair unranking serves the jet-coefficient table (dto_tdb_coef.hip.h) and
// those two kernels.  The TABLEAU is the statement of the scheme, tied forward-to-adjoint by tests/test_tdb_scheme_header.py.
// k_tdb_mfma (dto_tdb_mfma.hip: the forward loop, the Hessian's adjoint and the one-column adjoint of J' w) and k_tdb_kron_product
// (dto_tdb_kron.hip: its forward loop and its one-group adjoint) call it.  The six other stage loops (dto_tdb.hip: k_tdb forward
// and adjoint, k_tdb_product forward and adjoint; dto_tdb_kron.hip: k_tdb_kron forward and adjoint) spell tau, w_acc / w_tmp, cw / cu, the IN / OUT rotation and the stage update out: calling these helpers moved the
// register allocation of k_tdb_kron, and the shared forward / adjoint passes built on them made k_tdb slower at 4 states (DESIGN
// 4.21, last paragraph).  A change to the tableau below has to be repeated in those six loops.
#pragma once

#ifdef __HIPCC__
#define TDB_HD __host__ __device__
#else
#define TDB_HD
#endif

namespace dto {

// ---- counts.  theta = [u_k (m), t_k, dt_k, u_{k+1} (m, order 1 only)]; Q shared matrices B_q = G_j | H_cj, q = j (1 + nmod) + c
TDB_HD inline int tdb_num_params(int m, int order) { return m + 2 + (order ? m : 0); }
TDB_HD inline int tdb_num_pairs(int p) { return p * (p + 1) / 2; }
TDB_HD inline int tdb_num_shared(int m, int nmod) { return (m + 1) * (1 + nmod); }
// entries of the jet-coefficient table: one row of Q per jet of M (value, p first and p (p+1) / 2 second derivatives)
TDB_HD inline long tdb_table_entries(int m, int order, int nmod) {
    const int p = tdb_num_params(m, order);
    return (1L + p + tdb_num_pairs(p)) * tdb_num_shared(m, nmod);
}
constexpr int TDB_MAX_COEFS = 6144;   // the table's capacity (k_tdb keeps it in LDS)
TDB_HD inline bool tdb_table_fits(int m, int order, int nmod) { return tdb_table_entries(m, order, nmod) <= TDB_MAX_COEFS; }

// ---- parameter pairs a <= b < p, ranked row-major over the upper triangle
TDB_HD inline int tdb_pair_rank(int a, int b, int p) { return a * p - a * (a - 1) / 2 + (b - a); }
TDB_HD inline void tdb_pair_unrank(int e, int p, int* a, int* b) {
    int aa = 0;
    while (e >= p - aa) { e -= p - aa; ++aa; }
    *a = aa; *b = aa + e;
}

// ---- classical RK4 on tau in [0, 1] with steps of h.  Stage s of a step evaluates M at c_s = (0, 1/2, 1/2, 1), so stages 1 and 2
// share their time (and their jets).  Forward, with three buffers beside the accumulator:
//     stage 0: K = F(Y),  ACC = Y + h/6 K,  TA = Y + h/2 K        stage 2: K = F(TB), ACC += h/3 K,  TA = Y + h K
//     stage 1: K = F(TA), ACC += h/3 K,     TB = Y + h/2 K        stage 3: K = F(TA), Y = ACC + h/6 K
TDB_HD inline double tdb_stage_tau(int step, int stage, double h) { return (step + (stage == 0 ? 0.0 : (stage == 3 ? 1.0 : 0.5))) * h; }

TDB_HD inline double tdb_fwd_w_acc(int stage, double h) { return (stage == 0 || stage == 3) ? h / 6.0 : h / 3.0; }
TDB_HD inline double tdb_fwd_w_tmp(int stage, double h) { return stage == 2 ? h : 0.5 * h; }
struct TdbFwdStage { double tau, w_acc, w_tmp; };
TDB_HD inline TdbFwdStage tdb_fwd_stage(int step, int stage, double h) {
    return {tdb_stage_tau(step, stage, h), tdb_fwd_w_acc(stage, h), tdb_fwd_w_tmp(stage, h)};
}
TDB_HD inline bool tdb_fwd_new_jets(int stage) { return stage != 2; }
template <class T> TDB_HD inline T* tdb_fwd_in(int stage, T* Y, T* TA, T* TB) { return stage == 0 ? Y : (stage == 2 ? TB : TA); }
template <class T> TDB_HD inline T* tdb_fwd_out(int stage, T* Y, T* TA, T* TB) {
    return stage == 0 ? TA : (stage == 1 ? TB : (stage == 2 ? TA : Y));
}
// one entry's update: y0 its value at the start of the step, K the stage's right-hand side, acc / out its places in ACC and OUT
TDB_HD inline void tdb_fwd_update(int stage, double w_acc, double w_tmp, double y0, double K, double& acc, double& out) {
    if (stage == 0) { acc = y0 + w_acc * K; out = y0 + w_tmp * K; }
    else if (stage < 3) { acc += w_acc * K; out = y0 + w_tmp * K; }
    else out = acc + w_acc * K;
}

// The discrete adjoint of one step, stages 3 .. 0 (k4 first): kbar_s = cw w + cu ubar_{s+1}, ubar_s = M_s' kbar_s, w- = w + sum ubar_s
//     kbar_4 = h/6 w,  kbar_3 = h/3 w + h ubar_4,  kbar_2 = h/3 w + h/2 ubar_3,  kbar_1 = h/6 w + h/2 ubar_2
// Backward the shared time is that of stages 2 and 1.  ubar is not read at stage 3 (it holds nothing yet).
TDB_HD inline double tdb_bwd_cw(int stage, double h) { return (stage == 3 || stage == 0) ? h / 6.0 : h / 3.0; }
TDB_HD inline double tdb_bwd_cu(int stage, double h) { return stage == 3 ? 0.0 : (stage == 2 ? h : 0.5 * h); }
struct TdbBwdStage { double tau, cw, cu; };
TDB_HD inline TdbBwdStage tdb_bwd_stage(int step, int stage, double h) {
    return {tdb_stage_tau(step, stage, h), tdb_bwd_cw(stage, h), tdb_bwd_cu(stage, h)};
}
TDB_HD inline bool tdb_bwd_new_jets(int stage) { return stage != 1; }
TDB_HD inline double tdb_bwd_kbar(double cw, double cu, const double& w, const double& ubar) { return cw * w + (cu != 0.0 ? cu * ubar : 0.0); }

}  // namespace dto
