// dto_sweep_cache.h -- option reuse_forward_sweep: what the forward sweep buffer of one bilinear integrator (BilHost::fw) still holds
// for the cached point Z, as ONE record.  Plain C++ (no HIP header, no engine header): tests/test_sweep_cache_header.py builds it
// with g++ alone.  The record RECORDS and ANSWERS; which sweep form a callback takes from an answer is decided at the call sites
// in dto_engine.cpp, where the reasons are written down.
//   writing: one recorder per producer -- every sweep that leaves something in b.fw (or overwrites it) says so by name;
//   reading: only through at(same), a snapshot for one call.  `same` is that call's answer of same_point(): with same == false the
//            view holds nothing and has no plan, whatever the record says, so no read can leave the flag out.
#pragma once

namespace dto {

class SweepCache {
    struct State {
        int level = 0, steps = 0;         // Level; the steps of the sweep that stored ALL_TERMS
        int plan_q = 0, plan_dub = 0;     // the step budget the Jacobian's chain planned from its exact norms (q = 0: none)
        // the Taylor terms of the p column alone in fw.Zt ([term][Kpad][npad], one type per term): p_steps + 1 of them, valid counts
        // per block of p_nblk intervals in fw.nterms_p (the convergence blocks of the sweep that stored them)
        bool p_held = false;
        int p_steps = 0, p_nblk = 0;
    };

public:
    // the sums in fw.S / fw.GY, each level including the ones below it
    enum Level {
        NOTHING = 0,
        P_SUMS = 1,        // exp(A) x: the sums of the p column (S type 0)
        TANGENT_SUMS = 2,  // ... and of the d^j columns, and GY
        ALL_TERMS = 3,     // ... and every Taylor term of every column type in fw.Zt
    };

    // What one call may read: a SNAPSHOT taken by at(same) -- a recorder that runs later in the call does not show in it.  A count
    // that belongs to something not held is 0.
    class View {
    public:
        bool has_p_sums() const { return s_.level >= P_SUMS; }
        bool has_tangent_sums() const { return s_.level >= TANGENT_SUMS; }
        bool has_all_terms() const { return s_.level == ALL_TERMS; }
        int all_terms_steps() const { return has_all_terms() ? s_.steps : 0; }
        bool has_p_column() const { return s_.p_held; }
        int p_column_steps() const { return s_.p_held ? s_.p_steps : 0; }
        int p_column_nblk() const { return s_.p_held ? s_.p_nblk : 0; }
        bool has_plan() const { return s_.plan_q > 0; }
        int plan_rounds() const { return s_.plan_q; }
        int plan_budget() const { return has_plan() ? s_.plan_dub : 0; }

    private:
        friend class SweepCache;
        View(const State& s, bool same) : s_(same ? s : State{}) {}
        State s_;
    };
    View at(bool same) const { return View(s_, same); }

    // a new point, a changed option, a failed call: nothing of b.fw may be read again
    void invalidate() { s_.level = NOTHING; s_.p_held = false; s_.plan_q = 0; }

    // ---- recorders: `reuse` is the option, `steps` what run_sweep returned, `nblk` fw.nblk behind that sweep
    // eval_constraint, step budget read on the device (33..64 states, option off): no term kept, the host knows no step count
    void constraint_swept_on_device_plan(int nblk) { s_.level = NOTHING; set_p_column(false, 0, nblk); }
    // eval_constraint planned on the host; kept_p: the p column's terms were stored
    void constraint_swept(bool reuse, bool kept_p, int steps, int nblk) { s_.level = reuse ? P_SUMS : NOTHING; set_p_column(kept_p && reuse, steps, nblk); }
    // Jacobian, tangent columns alone on top of the stored p terms (which stay)
    void jacobian_swept_frozen() { s_.level = TANGENT_SUMS; }
    // Jacobian, every column; kept_all: every term of every type was stored.  That store, or a sweep of q > 1 rounds (other scale
    // factors), overwrites the p column's terms
    void jacobian_swept(bool reuse, bool kept_all, int q, int steps) {
        s_.level = reuse ? (kept_all ? ALL_TERMS : TANGENT_SUMS) : NOTHING;
        s_.steps = steps;
        if (kept_all || q > 1) s_.p_held = false;
    }
    // the Jacobian's chain planned its sweep from the exact norms of this point
    void chain_planned(int q, int d_ub) { s_.plan_q = q; s_.plan_dub = d_ub; }
    // Hessian, pairing path: the p column alone, terms stored -- the p sums are valid, the tangent sums are not
    void hessian_swept_p_column(bool reuse, int steps, int nblk) { s_.level = reuse ? P_SUMS : NOTHING; s_.steps = steps; set_p_column(reuse, steps, nblk); }
    // Hessian without pairing: second-order columns, scale factors of its own q
    void hessian_swept_second_order() { s_.level = NOTHING; s_.p_held = false; }
    // matrix-free J w / J' w: b.fw swept with the products' own column types
    void products_swept() { s_.level = NOTHING; s_.p_held = false; }

private:
    void set_p_column(bool held, int steps, int nblk) { s_.p_held = held; s_.p_steps = steps; s_.p_nblk = nblk; }
    State s_;
};

}  // namespace dto
