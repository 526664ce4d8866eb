// dto_create.cpp -- dto_create: builds the handle (dto_handle.h) from a problem description as a sequence of named stages.
//
// The sparsity structure follows the reference's exact order (src/solvers/evaluator.jl:119-209, closed forms of SURVEY.md §3.6 +
// a per-column prefix sum for the value-dependent constraint entries).  A structure-only handle (device < 0) runs the host part
// of the stages and touches no GPU.  Device allocations, uploads and the kernel launches of creation (the generator product
// norms, then the generator-subspace basis) keep one fixed order: the pairing store's decision reads the free device memory.
#include "dto_handle.h"
#include "dto_tdb_scheme.h"

#include <cmath>
#include <cstring>
#include <map>

using namespace dto;

namespace {

// ------------------------------------------------------------------------------------------
// structure
// ------------------------------------------------------------------------------------------

// Largest r dividing n with M == I_r (x) B for all m1 matrices of G and all mh of H (n x n column-major, compared with ==):
// off-diagonal blocks exactly zero, every diagonal block equal to the first.  1 if there is none.  (H: the carrier matrices of a
// time-dependent family; an all-zero matrix conforms to every r.)
int find_replicas(const double* G, int n, int m1, const double* H = nullptr, int mh = 0) {
    for (int r = n; r >= 2; --r) {
        if (n % r) continue;
        const int b = n / r;
        bool ok = true;
        for (int j = 0; j < m1 + mh && ok; ++j) {
            const double* M = j < m1 ? G + (size_t)j * n * n : H + (size_t)(j - m1) * n * n;
            for (int c = 0; c < n && ok; ++c) {
                const int bc = c / b;
                const double* col = M + (size_t)c * n;
                const double* first = M + (size_t)(c - bc * b) * n;
                for (int q = 0; q < n; ++q) {
                    const int bq = q / b;
                    if (bq != bc ? !(col[q] == 0.0) : !(col[q] == first[q - bq * b])) { ok = false; break; }
                }
            }
        }
        if (ok) return r;
    }
    return 1;
}

// the working block of a structured path: blocks below 16 rows are grouped while the group fits one MFMA row tile (I_g (x) B is a
// replicated block too)
void set_working_block(KKron& kk, int b, int r) {
    kk.b = b; kk.r = r;
    int grp = 1;
    if (b < 16)
        for (int c = 1; c <= r; ++c)
            if (r % c == 0 && c * b <= 16) grp = c;
    kk.bw = grp * b; kk.rw = r / grp; kk.bp = (kk.bw + 15) / 16 * 16;
}

// Does the fused one-workgroup-per-interval path (dto_small.hip) serve a bilinear integrator of n states and m drives?  n <= 16 with
// one wavefront, 17..32 with four, while the interval's matrices, generators and sweep columns fit the CU's LDS.  The one place
// that decides it: upload_generators and the grouping below ask here.
bool small_path_serves(int flags, int eval_hessian, int n, int m) {
    const int Tf = eval_hessian ? 1 + m + m * (m + 1) / 2 : 1 + m;
    return (flags & DTO_FLAG_GENERAL_PATH_ONLY) == 0 && n <= 32 && Tf <= MAX_TYPES && small_lds_bytes(n, m, Tf, 1 + m) <= 150 * 1024;
}

// DTO_FLAG_SHARED_GENERATORS: partition the bilinear integrators into groups with equal x_dim, control component and generators
// (compared with ==, as find_replicas does).  Host arithmetic on the descriptor: also on structure-only handles.
void find_share_groups(dto_handle* h, const dto_problem_desc* d) {
    for (int i = 0; i < d->n_integrators; ++i)
        if (h->integ_kind[i] == DTO_INTEGRATOR_BILINEAR) h->bil[h->integ_index[i]].list_pos = i;
    if (!(d->flags & DTO_FLAG_SHARED_GENERATORS)) return;
    // the path an integrator takes follows from x_dim, m and the flags -- equal for the members of a group -- except the structured
    // path, which also asks where state, controls and timestep lie: an integrator it serves is grouped with its like only
    for (int i = 0; i < d->n_integrators; ++i) {
        if (h->integ_kind[i] != DTO_INTEGRATOR_BILINEAR) continue;
        const int bi = h->integ_index[i];
        if (h->bil[bi].share_leader >= 0) continue;  // a member of an earlier group
        const dto_integrator_desc& a = d->integrators[i];
        const size_t len = (size_t)(a.u_dim + 1) * a.x_dim * a.x_dim;
        std::vector<int> members{bi};
        for (int j = i + 1; j < d->n_integrators; ++j) {
            if (h->integ_kind[j] != DTO_INTEGRATOR_BILINEAR) continue;
            const int bj = h->integ_index[j];
            const dto_integrator_desc& c = d->integrators[j];
            if (h->bil[bj].share_leader >= 0 || c.x_dim != a.x_dim || c.u_dim != a.u_dim || (a.u_dim > 0 && c.u_off != a.u_off) ||
                h->bil[bj].kron != h->bil[bi].kron)
                continue;
            bool eq = true;
            for (size_t e = 0; e < len && eq; ++e) eq = a.G[e] == c.G[e];
            if (eq) members.push_back(bj);
        }
        if (members.size() < 2) continue;
        const bool active = !h->bil[bi].kron && !small_path_serves(d->flags, d->eval_hessian, a.x_dim, a.u_dim) && members.size() - 1 <= (size_t)SHARE_MAX_FOLLOWERS;
        for (int mb : members) {
            h->bil[mb].share_leader = bi;
            h->bil[mb].share_size = (int)members.size();
            h->bil[mb].share_active = active;
        }
        if (active) h->bil[bi].share_followers.assign(members.begin() + 1, members.end());
    }
}

// The same flag on DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR integrators: groups of equal x_dim, control and time component, scheme
// (order, substeps), modulations and matrices G_j, H_cj (==).  Never mixed with the bilinear kind.  A group is active when its
// members run on k_tdb_mfma; its launches take at most `share_cap` members, the largest count whose scratch slot stays within
// TDB_SHARE_SLOT_BYTES per resident workgroup (the slot is 4 np Ctot + np^2 + the U_q columns, tdb_mfma_scratch_doubles).
constexpr size_t TDB_SHARE_SLOT_BYTES = (size_t)8 << 20;

bool same_time_dependent_system(const dto_integrator_desc& a, const dto_integrator_desc& c) {
    if (c.x_dim != a.x_dim || c.u_dim != a.u_dim || (a.u_dim > 0 && c.u_off != a.u_off) || c.t_off != a.t_off ||
        c.spline_order != a.spline_order || c.substeps != a.substeps || c.n_mod != a.n_mod)
        return false;
    for (int m = 0; m < a.n_mod; ++m)
        if (a.mod_kind[m] != c.mod_kind[m] || !(a.mod_omega[m] == c.mod_omega[m])) return false;
    const size_t len = (size_t)(a.u_dim + 1) * a.x_dim * a.x_dim;
    for (size_t e = 0; e < len; ++e)
        if (!(a.G[e] == c.G[e])) return false;
    for (size_t e = 0; e < len * (size_t)a.n_mod; ++e)
        if (!(a.H[e] == c.H[e])) return false;
    return true;
}

void find_time_dependent_share_groups(dto_handle* h, const dto_problem_desc* d) {
    for (int i = 0; i < d->n_integrators; ++i)
        if (h->integ_kind[i] == DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR) h->tdb[h->integ_index[i]].list_pos = i;
    if (!(d->flags & DTO_FLAG_SHARED_GENERATORS)) return;
    for (int i = 0; i < d->n_integrators; ++i) {
        if (h->integ_kind[i] != DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR) continue;
        const int ti = h->integ_index[i];
        if (h->tdb[ti].share_leader >= 0) continue;  // a member of an earlier group
        std::vector<int> members{ti};
        for (int j = i + 1; j < d->n_integrators; ++j) {
            if (h->integ_kind[j] != DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR) continue;
            const int tj = h->integ_index[j];
            // (a structured member groups with its like only; the dense paths follow from x_dim)
            if (h->tdb[tj].share_leader < 0 && h->tdb[tj].kron == h->tdb[ti].kron && same_time_dependent_system(d->integrators[i], d->integrators[j]))
                members.push_back(tj);
        }
        if (members.size() < 2) continue;
        const TdbHost& lead = h->tdb[ti];
        int cap = 1;
        if (lead.mfma && !lead.kron)
            for (int g = 2; g <= std::min<int>((int)members.size(), TDB_SHARE_MAX); ++g) {
                size_t slot = std::max(tdb_mfma_scratch_doubles(lead.k, 0, g), tdb_mfma_scratch_doubles(lead.k, 1, g));
                if (d->eval_hessian) slot = std::max(slot, tdb_mfma_scratch_doubles(lead.k, 2, g));
                if (slot * sizeof(double) > TDB_SHARE_SLOT_BYTES) break;
                cap = g;
            }
        for (int mb : members) {
            h->tdb[mb].share_leader = ti;
            h->tdb[mb].share_size = (int)members.size();
            h->tdb[mb].share_active = cap >= 2;
            h->tdb[mb].share_cap = cap;
        }
        if (cap >= 2) h->tdb[ti].share_members = members;
    }
}

double con_jac_value(const ConHost& c, const double* zk, int comp_i) {
    if (c.k.kind == DTO_CONSTRAINT_QUADFORM_MINUS_C) {  // 2 (M v)_c, summed over j ascending with an unfused multiply-add: the
        const size_t n = c.comps.size();                // arithmetic of the device's row walk (dto_quadform.hip, qf_row)
        double y = 0.0;
        {
#pragma clang fp contract(off)
            for (size_t j = 0; j < n; ++j) y = y + c.M[(size_t)comp_i + n * j] * zk[c.comps[j]];
        }
        return 2.0 * y;
    }
    double s = 0.0;
    for (int q : c.comps) s += zk[q] * zk[q];
    const double v = zk[c.comps[comp_i]];
    return c.k.kind == DTO_CONSTRAINT_NORM_MINUS_C ? v / std::sqrt(s) : 2.0 * v;
}

void build_structure(dto_handle* h, const double* Z0) {
    const int64_t nv = h->n_vars;
    // constraint pattern = numeric Jacobian at Z0, exact zeros not stored (evaluator.jl:136)
    std::vector<std::pair<int64_t, int64_t>> ent;
    for (auto& c : h->con) {
        for (int64_t i = 0; i < c.n_times_total; ++i) {
            const int64_t kn = c.times0[i];
            const double* zk = Z0 + kn * h->z;
            for (size_t q = 0; q < c.comps.size(); ++q) {
                if (c.external) {
                    for (int r = 0; r < c.g_dim; ++r)
                        if (c.jac0[((size_t)i * c.comps.size() + q) * c.g_dim + r] != 0.0)
                            ent.emplace_back(kn * h->z + c.comps[q], c.row_off + i * c.g_dim + r);
                    continue;
                }
                const double v = con_jac_value(c, zk, (int)q);
                if (v != 0.0) ent.emplace_back(kn * h->z + c.comps[q], c.row_off + i);
            }
        }
    }
    std::sort(ent.begin(), ent.end());
    ent.erase(std::unique(ent.begin(), ent.end()), ent.end());
    h->con_cols.resize(ent.size());
    h->con_rows.resize(ent.size());
    std::vector<int32_t> extra(nv, 0);
    for (size_t i = 0; i < ent.size(); ++i) {
        h->con_cols[i] = ent[i].first;
        h->con_rows[i] = ent[i].second;
        extra[ent[i].first]++;
    }
    h->colptr.assign(nv + 1, 0);
    const SlabDims L = slab_dims(h);
    const int64_t z = h->z;
    // (global columns, kn >= N: only NonlinearGlobalConstraint rows)
    for (int64_t c = 0; c < nv; ++c) h->colptr[c + 1] = h->colptr[c] + jac_con_off(L, c / z) + extra[c];
    h->jac_nnz = h->colptr[nv];
    h->hess_block_nnz = hess_block_start(L, h->N);  // N tri + K z^2: evaluator.jl:201-202 on the block pattern
    // tail: entries whose column is a global variable (global columns follow every knot column in the CSC order).
    // GlobalObjective / GlobalKnotPointObjective mark their whole index block (global_objectives.jl:89-101, 277-300),
    // NonlinearGlobalConstraint contributes the non-zeros of its Hessian at mu = ones (evaluator.jl:166)
    std::vector<std::vector<int64_t>> rows(h->gd);
    const int64_t g0 = h->N * z;
    for (auto& e : h->ext_obj) {
        if (!e.global) continue;
        for (int gb : e.gcomps) {
            for (int64_t t : e.times0)
                if (t < h->N)
                    for (int ca : e.comps) rows[gb].push_back(t * z + ca);
            for (int ga : e.gcomps)
                if (ga <= gb) rows[gb].push_back(g0 + ga);
        }
    }
    for (auto& c : h->con) {
        if (!c.global) continue;
        const size_t ng = c.comps.size();
        for (size_t b = 0; b < ng; ++b)
            for (size_t a = 0; a < ng; ++a)
                if (c.comps[a] <= c.comps[b] && c.hess0[a + ng * b] != 0.0) rows[c.comps[b]].push_back(g0 + c.comps[a]);
    }
    h->tail_colptr.assign(h->gd + 1, 0);
    h->tail_rows.clear();
    for (int j = 0; j < h->gd; ++j) {
        std::sort(rows[j].begin(), rows[j].end());
        rows[j].erase(std::unique(rows[j].begin(), rows[j].end()), rows[j].end());
        h->tail_rows.insert(h->tail_rows.end(), rows[j].begin(), rows[j].end());
        h->tail_colptr[j + 1] = (int64_t)h->tail_rows.size();
    }
    h->hess_nnz = h->hess_block_nnz + (int64_t)h->tail_rows.size();
}

// ------------------------------------------------------------------------------------------
// workspaces of a bilinear integrator on the general path
// ------------------------------------------------------------------------------------------

void alloc_sweep(dto_handle* h, BilHost& b, SweepBuf& w, int T, bool with_W) {
    const int npad = b.k.npad;
    w.npad = npad;
    w.T_alloc = T;
    w.TN = (npad % 128 == 0) ? 128 : 64;
    w.nblk = w.TN;
    int64_t nint = std::max<int64_t>(h->P.n_int, 1);
    w.Kpad = (int)(((nint + w.TN - 1) / w.TN) * w.TN);
    const size_t typesz = (size_t)w.Kpad * npad;
    w.Z[0] = own(h, dalloc<double>(typesz * T));
    w.Z[1] = own(h, dalloc<double>(typesz * T));
    w.S = own(h, dalloc<double>(typesz * T));
    w.GY = own(h, dalloc<double>(typesz));
    w.W = with_W ? own(h, dalloc<double>(typesz * (b.k.m + 1))) : nullptr;
    w.scaleA = own(h, dalloc<double>((size_t)(b.k.m + 1) * w.Kpad));
    w.scaleU = own(h, dalloc<double>((size_t)(b.k.m + 1) * w.Kpad));
    w.scaleE = own(h, dalloc<double>((size_t)2 * w.Kpad));
    w.termnorm = own(h, dalloc<unsigned long long>((size_t)3 * T * w.Kpad));
    w.sumnorm = own(h, dalloc<unsigned long long>((size_t)T * w.Kpad));
    w.active = own(h, dalloc<int32_t>(w.Kpad / w.TN));
    w.stats = own(h, dalloc<int32_t>(4));
    HIP_CHECK(hipMemset(w.stats, 0, 4 * sizeof(int32_t)));
    // padding columns/rows must be finite zeros from the start
    HIP_CHECK(hipMemset(w.Z[0], 0, typesz * T * sizeof(double)));
    HIP_CHECK(hipMemset(w.Z[1], 0, typesz * T * sizeof(double)));
    HIP_CHECK(hipMemset(w.S, 0, typesz * T * sizeof(double)));
    HIP_CHECK(hipMemset(w.GY, 0, typesz * sizeof(double)));
}

// multisets of size r over {0..m} as sorted tuples, lexicographic
void enum_multisets(int m1, int r, std::vector<int>& cur, int start, std::vector<std::vector<int>>& out) {
    if ((int)cur.size() == r) { out.push_back(cur); return; }
    for (int i = start; i < m1; ++i) {
        cur.push_back(i);
        enum_multisets(m1, r, cur, i, out);
        cur.pop_back();
    }
}

// S_alpha = sum over distinct first letters i of alpha of G_i * S_(alpha minus i): built once at create with
// the engine's own batched GEMM (one product per (alpha, i)).
void build_basis(dto_handle* h, BilHost& b, int cap) {
    const int m1 = b.k.m + 1, npad = b.k.npad;
    const size_t nn = (size_t)npad * npad;
    std::vector<std::vector<std::vector<int>>> sets(5);
    std::vector<std::map<std::vector<int>, int>> index(5);
    for (int r = 1; r <= 4; ++r) {
        std::vector<int> cur;
        enum_multisets(m1, r, cur, 0, sets[r]);
        for (size_t a = 0; a < sets[r].size(); ++a) index[r][sets[r][a]] = (int)a;
    }
    double* tmp = own(h, dalloc<double>(nn));
    std::vector<double*> S(5, nullptr);
    S[1] = const_cast<double*>(b.k.G);
    for (int r = 2; r <= 4; ++r) {
        const int cnt = (int)sets[r].size(), cntpad = ((cnt + 15) / 16) * 16;
        S[r] = own(h, dalloc<double>(nn * cntpad));
        HIP_CHECK(hipMemsetAsync(S[r], 0, nn * cntpad * sizeof(double), h->stream));
        std::vector<int32_t> idx;
        for (int a = 0; a < cnt; ++a) {
            const std::vector<int>& al = sets[r][a];
            for (int v : al) idx.push_back(v);
            int last = -1;
            for (size_t p = 0; p < al.size(); ++p) {
                const int i = al[p];
                if (i == last) continue;  // distinct first letters only
                last = i;
                std::vector<int> rest = al;
                rest.erase(rest.begin() + p);
                const double* prev = S[r - 1] + (size_t)index[r - 1][rest] * nn;
                launch_bgemm_plain(h->stream, npad, 1, b.k.G + (size_t)i * nn, prev, tmp);
                launch_add(h->stream, S[r] + (size_t)a * nn, tmp, (int64_t)nn);
            }
        }
        BasisSet& bs = b.basis[r - 2];
        bs.r = r; bs.cnt = cnt; bs.cntpad = cntpad; bs.S = S[r];
        bs.idx = own(h, dupload(idx));
        const int cappad = ((cap + 127) / 128) * 128;
        bs.coef = own(h, dalloc<double>((size_t)cappad * cntpad));
    }
    {
        // concatenation [I | G_0..G_m | S2 | S3 | S4] for the factor K
        int cnt = 1 + m1;
        for (int r = 2; r <= 4; ++r) cnt += (int)sets[r].size();
        const int cntpad = ((cnt + 15) / 16) * 16;
        double* Sall = own(h, dalloc<double>(nn * cntpad));
        HIP_CHECK(hipMemsetAsync(Sall, 0, nn * cntpad * sizeof(double), h->stream));
        std::vector<double> eye(nn, 0.0);
        for (int i = 0; i < b.k.n; ++i) eye[(size_t)i * npad + i] = 1.0;  // identity on the un-padded block only
        HIP_CHECK(hipMemcpyAsync(Sall, eye.data(), nn * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        std::vector<int32_t> idx;
        size_t col = 1;
        for (int q = 0; q < 4; ++q) idx.push_back(-1);
        for (int r = 1; r <= 4; ++r) {
            HIP_CHECK(hipMemcpyAsync(Sall + col * nn, S[r], nn * sets[r].size() * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            col += sets[r].size();
            for (auto& al : sets[r]) {
                for (int q = 0; q < 4; ++q) idx.push_back(q < r ? al[q] : -1);
            }
        }
        BasisSet& bs = b.basis_all;
        bs.r = 4; bs.cnt = cnt; bs.cntpad = cntpad; bs.S = Sall;
        bs.idx = own(h, dupload(idx));
        const int cappad = ((cap + 127) / 128) * 128;
        bs.coef = own(h, dalloc<double>((size_t)cappad * cntpad));
    }
    HIP_CHECK(hipStreamSynchronize(h->stream));
    b.use_basis = true;
}

void alloc_chain(dto_handle* h, BilHost& b, int cap) {
    const size_t nn = (size_t)b.k.npad * b.k.npad;
    for (int i = 0; i < 9; ++i) b.chain.W[i] = own(h, dalloc<double>(nn * cap));
    b.chain.norms = own(h, dalloc<double>((size_t)cap * 4));
    b.chain.colsum = own(h, dalloc<double>((size_t)3 * cap * b.k.npad * (b.k.npad / 64)));  // [set][interval][column][64-row chunk]
    if (!b.d_hump) b.d_hump = own(h, dalloc<unsigned long long>(8));
    b.chain.coef = own(h, dalloc<double>((size_t)cap * COEF_STRIDE));
    b.chain.s = own(h, dalloc<int32_t>(cap));
    b.chain.s3 = own(h, dalloc<int32_t>(cap));
    b.chain.smax = own(h, dalloc<int32_t>(8));
    HIP_CHECK(hipMemset(b.chain.smax, 0, 8 * sizeof(int32_t)));
    b.chain.d2max = reinterpret_cast<unsigned long long*>(b.chain.smax + 2);
    b.chain_cap = cap;
}

int chunk_size(const dto_handle* h, int npad) {
    // workspace budget for the 9 chain matrices (option "chain_chunk" lowers the chunk per call)
    const double budget = 40e9;   // (1024 states x 500 knots, the configs[4] share, in ONE chunk: 37.7 GB)
    int c = (int)(budget / (9.0 * npad * (double)npad * 8.0));
    c = std::max(8, (c / 8) * 8);
    return (int)std::min<int64_t>(c, std::max<int64_t>(h->P.n_int, 1));
}

// ------------------------------------------------------------------------------------------
// fragments the stages share
// ------------------------------------------------------------------------------------------

// is listing i the last one of times[0..n) that names its knot?
template <class T>
bool last_listing_of_knot(const T* times, int64_t n, int64_t i) {
    for (int64_t i2 = i + 1; i2 < n; ++i2)
        if (times[i2] == times[i]) return false;
    return true;
}

// a description's 1-based knot, checked against 1..N, as a 0-based one
int64_t knot0(int64_t time1, int64_t N, const char* what) {
    if (time1 < 1 || time1 > N) throw HipError{std::string(what) + ": time out of range"};
    return time1 - 1;
}

void check_comps(const std::vector<int32_t>& comps, int bound, const char* msg) {
    for (int q : comps)
        if (q < 0 || q >= bound) throw HipError{msg};
}

// does this handle own knot kn (0-based)?
bool owns_knot(const dto_handle* h, int64_t kn) { return kn >= h->P.kn_lo && kn < h->P.kn_lo + h->P.n_knots; }

// the leading n x n blocks of `count` column-major ld x ld matrices, zero-padded to np x np, and their transposes (dst and dstT
// arrive zeroed)
void pad_with_transpose(const double* src, size_t count, size_t ld, size_t n, size_t np, double* dst, double* dstT) {
    for (size_t j = 0; j < count; ++j)
        for (size_t c = 0; c < n; ++c)
            for (size_t r = 0; r < n; ++r) {
                const double v = src[j * ld * ld + c * ld + r];
                dst[j * np * np + c * np + r] = v;
                dstT[j * np * np + r * np + c] = v;
            }
}

// doubles of one scratch slot: what the first-order callbacks need, the second-order ones too with a Hessian, rounded up to even
size_t scratch_stride(size_t first, size_t second, bool hessian) { return (std::max(first, hessian ? second : (size_t)0) + 1) & ~(size_t)1; }

// ------------------------------------------------------------------------------------------
// stages of dto_create, in the order they run.  A structure-only handle (device < 0) takes the host part of each stage up to
// place_external_objectives and none after it.
// ------------------------------------------------------------------------------------------

// what is checked before a handle exists; nullptr if the description passes
const char* check_desc(const dto_problem_desc* d) {
    if (d->abi_version != DTO_ABI_VERSION) return "dto_create: ABI version mismatch";
    if (d->N < 2) return "dto_create: need at least 2 knots";
    if (d->z < 1 || d->gd < 0) return "dto_create: bad dimensions";
    if (d->dt_idx < 0 || d->dt_idx >= d->z) return "dto_create: the timestep must be a trajectory component (bilinear_integrator.jl:123)";
    if (!d->Z0) return "dto_create: Z0 is required (constraint patterns are taken at Z0)";
    if (d->device >= 0) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return "dto_create: no HIP device available (the engine has no CPU fallback)";
        if (d->device >= ndev) return "dto_create: bad device ordinal";
    }
    return nullptr;
}

void open_device(dto_handle* h) {
    HIP_CHECK(hipSetDevice(h->device));
    HIP_CHECK(hipStreamCreate(&h->stream));
    HIP_CHECK(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&h->stream_rb, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&h->ev_rb, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&h->ev_zero, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&h->ev_stats, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&h->ev_chain, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming));
    HIP_CHECK(hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, h->device));
    HIP_CHECK(sweep_fused_prepare());
    HIP_CHECK(sweep_cluster_prepare());
    HIP_CHECK(sweep_gs_prepare());
    HIP_CHECK(chain64_prepare());
}

void set_dimensions(dto_handle* h, const dto_problem_desc* d) {
    h->N = d->N; h->K = d->N - 1; h->z = d->z; h->gd = d->gd; h->dt_idx = d->dt_idx;
    h->eval_hessian = d->eval_hessian;
    h->n_vars = (int64_t)d->z * d->N + d->gd;
    h->k_lo = d->k_lo > 0 ? d->k_lo : 1;
    h->k_hi = d->k_hi > 0 ? d->k_hi : d->N;
    if (h->k_lo > h->k_hi || h->k_hi > h->N) throw HipError{"dto_create: bad knot shard"};
}

// ---- integrators.  `pre`: states of the integrators listed before this one; `row`: its first global row.

void check_bilinear(const dto_integrator_desc& s, int z) {
    if (s.u_dim < 0 || s.u_dim > MAX_DRIVES) throw HipError{"bilinear integrator: supports 0..7 drives"};
    if (s.u_dim > 0 && (s.u_off < 0 || s.u_off + s.u_dim > z)) throw HipError{"bilinear integrator: bad control range"};
    if (!s.G) throw HipError{"bilinear integrator: G is null"};
}

// DTO_FLAG_BLOCK_GENERATORS: the replicated blocks of the generators, and whether the structured path (dto_kron.hip) serves them
void find_blocks(BilHost& b, const dto_problem_desc* d, const dto_integrator_desc& s) {
    const int n = s.x_dim;
    b.kr = find_replicas(s.G, n, s.u_dim + 1);
    b.kb = n / b.kr;
    KKron& kk = b.kk;
    set_working_block(kk, b.kb, b.kr);
    // the structured kernel gives every Hessian entry of the block one writer: state, controls and timestep apart
    const bool apart = (s.u_dim == 0 || s.u_off + s.u_dim <= s.x_off || s.u_off >= s.x_off + n) &&
                       (d->dt_idx < s.x_off || d->dt_idx >= s.x_off + n) &&
                       (s.u_dim == 0 || d->dt_idx < s.u_off || d->dt_idx >= s.u_off + s.u_dim);
    b.kron = b.kr >= 2 && b.kb <= 64 && n > 32 && apart && kron_supported(kk, s.u_dim, d->eval_hessian != 0);
}

// the generators in the layout of the path that serves the integrator: working blocks (structured), or the padded matrices and,
// on the fused small path, the compact ones as well
void upload_generators(dto_handle* h, const dto_problem_desc* d, const dto_integrator_desc& s, BilHost& b) {
    const int n = s.x_dim, m = s.u_dim, m1 = m + 1;
    if (b.kron) {
        const size_t bp = b.kk.bp;
        std::vector<double> Bm(m1 * bp * bp, 0.0), BmT(m1 * bp * bp, 0.0);
        pad_with_transpose(s.G, m1, n, b.kk.bw, bp, Bm.data(), BmT.data());
        b.kk.Bm = own(h, dupload(Bm));
        b.kk.BmT = own(h, dupload(BmT));
        HIP_CHECK(kron_prepare());
        return;
    }
    const size_t np = b.k.npad;
    // (+ 16 zero columns: the fused sweep streams the generators a few k-steps ahead, past the last one)
    std::vector<double> G(m1 * np * np + 16 * np, 0.0), GT(m1 * np * np + 16 * np, 0.0);
    pad_with_transpose(s.G, m1, n, n, np, G.data(), GT.data());
    b.k.G = own(h, dupload(G));
    b.k.GT = own(h, dupload(GT));
    if (small_path_serves(d->flags, d->eval_hessian, n, m)) {
        const int Tf = d->eval_hessian ? 1 + m + m * (m + 1) / 2 : 1 + m;
        b.small = true;
        // worst-case dynamic LDS of this handle's fused kernel, opted into on THIS device
        // (the J w mode sweeps one forward column more than a Jacobian-only handle's other calls)
        HIP_CHECK(small_prepare(std::max(small_lds_bytes(n, m, Tf, 1 + m), small_lds_bytes(n, m, 2 + m, 1))));
        b.d_Gs = own(h, dupload(std::vector<double>(s.G, s.G + (size_t)m1 * n * n)));
    }
}

void add_bilinear(dto_handle* h, const dto_problem_desc* d, const dto_integrator_desc& s, int pre, int64_t row) {
    check_bilinear(s, d->z);
    BilHost b;
    b.k.n = s.x_dim; b.k.m = s.u_dim; b.k.npad = pad64(s.x_dim);
    b.k.x_off = s.x_off; b.k.u_off = s.u_off; b.k.pre = pre; b.k.row_off = row;
    const int n = s.x_dim, m1 = s.u_dim + 1;
    b.g1.assign(m1, 0.0);
    for (int j = 0; j < m1; ++j)
        for (int c = 0; c < n; ++c) {
            double cs = 0.0;
            for (int r = 0; r < n; ++r) cs += std::fabs(s.G[(size_t)j * n * n + (size_t)c * n + r]);
            b.g1[j] = std::max(b.g1[j], cs);
        }
    b.kb = n; b.kr = 1;
    if (d->flags & DTO_FLAG_BLOCK_GENERATORS) find_blocks(b, d, s);
    if (!h->structure_only) upload_generators(h, d, s, b);
    h->integ_index.push_back((int)h->bil.size());
    h->bil.push_back(std::move(b));
}

void add_derivative(dto_handle* h, const dto_problem_desc* d, const dto_integrator_desc& s, int pre, int64_t row) {
    if (s.u_off < 0 || s.u_off + s.x_dim > d->z) throw HipError{"derivative integrator: bad derivative range"};
    KDer k{};
    k.d = s.x_dim; k.x_off = s.x_off; k.xdot_off = s.u_off; k.pre = pre; k.row_off = row;
    h->integ_index.push_back((int)h->der.size());
    h->der.push_back(k);
}

void upload_time_dependent(dto_handle* h, const dto_integrator_desc& s, TdbHost& t) {
    const size_t n = s.x_dim, nn = n * n, m1 = (size_t)s.u_dim + 1;
    // (the structured kernel reads the blocks below, not the n x n matrices)
    if (!t.kron) t.k.G = own(h, dupload(std::vector<double>(s.G, s.G + m1 * nn)));
    if (s.n_mod > 0) {
        if (!t.kron) t.k.H = own(h, dupload(std::vector<double>(s.H, s.H + (size_t)s.n_mod * m1 * nn)));
        t.k.mod_kind = own(h, dupload(std::vector<int32_t>(s.mod_kind, s.mod_kind + s.n_mod)));
        t.k.mod_omega = own(h, dupload(std::vector<double>(s.mod_omega, s.mod_omega + s.n_mod)));
    }
    if (t.kron) {
        // the working blocks of B_q (the leading bw x bw block of each matrix), same order, and their transposes
        const size_t bp = t.kk.bp, nm1 = (size_t)s.n_mod + 1;
        std::vector<double> Bm(m1 * nm1 * bp * bp, 0.0), BmT(Bm.size(), 0.0);
        for (size_t j = 0; j < m1; ++j)
            for (size_t c = 0; c < nm1; ++c)
                pad_with_transpose(c == 0 ? s.G + j * nn : s.H + ((c - 1) * m1 + j) * nn, 1, n, t.kk.bw, bp, Bm.data() + (j * nm1 + c) * bp * bp,
                                   BmT.data() + (j * nm1 + c) * bp * bp);
        t.kk.Bm = own(h, dupload(Bm));
        t.kk.BmT = own(h, dupload(BmT));
    }
    if (t.mfma) {
        // B_q, q = j (1 + n_mod) + c (c = 0: G_j, c >= 1: H_{c-1, j}), zero-padded, and their transposes
        const size_t np = (size_t)tdb_mfma_npad(s.x_dim), nm1 = (size_t)s.n_mod + 1;
        std::vector<double> Bp(m1 * nm1 * np * np, 0.0), BpT(Bp.size(), 0.0);
        for (size_t j = 0; j < m1; ++j)
            for (size_t c = 0; c < nm1; ++c)
                pad_with_transpose(c == 0 ? s.G + j * nn : s.H + ((c - 1) * m1 + j) * nn, 1, n, n, np, Bp.data() + (j * nm1 + c) * np * np,
                                   BpT.data() + (j * nm1 + c) * np * np);
        t.d_Bp = own(h, dupload(Bp));
        t.d_BpT = own(h, dupload(BpT));
    }
}

// DTO_FLAG_BLOCK_GENERATORS on a time-dependent family: the replicated blocks shared by every G_j and H_cj, and whether the
// structured path (dto_tdb_kron.hip) serves the integrator
void find_blocks_time_dependent(TdbHost& t, const dto_problem_desc* d, const dto_integrator_desc& s) {
    const int n = s.x_dim, m1 = s.u_dim + 1;
    t.kr = find_replicas(s.G, n, m1, s.H, s.n_mod > 0 ? s.n_mod * m1 : 0);
    t.kb = n / t.kr;
    set_working_block(t.kk, t.kb, t.kr);
    // the structured kernel assigns its entries of the staged blocks: state, controls, time and timestep apart
    auto in_x = [&](int q) { return q >= s.x_off && q < s.x_off + n; };
    auto in_u = [&](int q) { return s.u_dim > 0 && q >= s.u_off && q < s.u_off + s.u_dim; };
    const bool apart = (s.u_dim == 0 || s.u_off + s.u_dim <= s.x_off || s.u_off >= s.x_off + n) && !in_x(s.t_off) && !in_u(s.t_off) &&
                       !in_x(d->dt_idx) && !in_u(d->dt_idx) && s.t_off != d->dt_idx;
    t.kron = apart && tdb_kron_supported(t.k, t.kk);
}

void add_time_dependent(dto_handle* h, const dto_problem_desc* d, const dto_integrator_desc& s, int pre, int64_t row) {
    if (s.u_dim < 0 || s.u_dim > MAX_DRIVES) throw HipError{"time-dependent bilinear integrator: supports 0..7 drives"};
    if (s.u_dim > 0 && (s.u_off < 0 || s.u_off + s.u_dim > d->z)) throw HipError{"time-dependent bilinear integrator: bad control range"};
    if (s.t_off < 0 || s.t_off >= d->z) throw HipError{"time-dependent bilinear integrator: bad time component"};
    if (s.spline_order != 0 && s.spline_order != 1) throw HipError{"Unsupported spline order (0 or 1)"};
    if (!s.G || (s.n_mod > 0 && (!s.H || !s.mod_kind || !s.mod_omega))) throw HipError{"time-dependent bilinear integrator: G / H / modulation arrays are null"};
    TdbHost t;
    t.k.n = s.x_dim; t.k.m = s.u_dim; t.k.x_off = s.x_off; t.k.u_off = s.u_off; t.k.t_off = s.t_off;
    t.k.order = s.spline_order; t.k.substeps = s.substeps; t.k.nmod = s.n_mod; t.k.row_off = row;
    t.kb = s.x_dim; t.kr = 1;
    if (d->flags & DTO_FLAG_BLOCK_GENERATORS) find_blocks_time_dependent(t, d, s);
    // 1..64 states: k_tdb; 65..256 states: k_tdb_mfma; replicated blocks, 33..512 states: k_tdb_kron; the refusal names the limit
    // that was hit
    if (!t.kron) {
        if (t.kr >= 2 && t.kb <= 64 && s.x_dim > 512)
            throw HipError{"time-dependent bilinear integrator: the structured path (replicated-block generators) takes up to 512 states"};
        if (const char* why = tdb_mfma_refusal(t.k)) throw HipError{why};
        t.mfma = tdb_mfma_supported(t.k);
        if (!t.mfma && !tdb_supported(t.k)) throw HipError{"time-dependent bilinear integrator: outside the device kernels' range (1..256 states, substeps >= 1, coefficient table)"};
    }
    for (int c = 0; c < s.n_mod; ++c)
        if (s.mod_kind[c] != 1 && s.mod_kind[c] != 2) throw HipError{"time-dependent bilinear integrator: mod_kind is 1 (cos) or 2 (sin)"};
    t.place.d = s.x_dim; t.place.pre = pre; t.place.row_off = row;
    if (!h->structure_only) upload_time_dependent(h, s, t);
    h->integ_index.push_back((int)h->tdb.size());
    h->tdb.push_back(t);
}

void add_external_integrator(dto_handle* h, const dto_problem_desc* d, const dto_integrator_desc& s, int pre, int64_t row) {
    KExtInt e{};
    e.d = s.x_dim; e.pre = pre; e.row_off = row;
    h->integ_index.push_back((int)h->ext_int.size());
    h->ext_int.push_back(e);
    ExtSlot sl;
    sl.len[0] = (size_t)s.x_dim * h->K;
    sl.len[1] = (size_t)s.x_dim * 2 * d->z * h->K;
    sl.len[2] = (size_t)4 * d->z * d->z * h->K;
    h->ext.push_back(sl);
}

// rows stacked in list order (evaluator.jl:211-217)
void add_integrators(dto_handle* h, const dto_problem_desc* d) {
    int pre = 0;
    int64_t row = 0;
    for (int i = 0; i < d->n_integrators; ++i) {
        const dto_integrator_desc& s = d->integrators[i];
        if (s.x_dim < 1 || (s.kind != DTO_INTEGRATOR_EXTERNAL && (s.x_off < 0 || s.x_off + s.x_dim > d->z)))
            throw HipError{"integrator: bad state range"};
        h->integ_kind.push_back(s.kind);
        h->integ_dim.push_back(s.x_dim);
        h->integ_row_off.push_back(row);
        switch (s.kind) {
            case DTO_INTEGRATOR_BILINEAR: add_bilinear(h, d, s, pre, row); break;
            case DTO_INTEGRATOR_DERIVATIVE: add_derivative(h, d, s, pre, row); break;
            case DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR: add_time_dependent(h, d, s, pre, row); break;
            case DTO_INTEGRATOR_EXTERNAL: add_external_integrator(h, d, s, pre, row); break;
            default: throw HipError{"unknown integrator kind"};
        }
        pre += s.x_dim;
        row += (int64_t)s.x_dim * h->K;
    }
    h->D = pre;
    h->n_dyn = row;
    h->n_ext_int = (int)h->ext_int.size();
}

// ---- constraints and host-evaluated objective terms: what they are, their rows and their dto_set_external slots

// NonlinearGlobalConstraint: one listing at the pseudo-knot N whose "components" are global_data entries
ConHost global_constraint(const dto_problem_desc* d, const dto_constraint_desc& s) {
    if (s.n_comps < 1 || !s.comps || s.g_dim < 1 || !s.jac0 || !s.hess0)
        throw HipError{"global constraint: comps, g_dim, jac0 and hess0 are required"};
    ConHost c;
    c.k.kind = s.kind; c.k.n_comps = s.n_comps; c.equality = s.equality;
    c.external = true; c.global = true; c.g_dim = s.g_dim;
    c.k.g_dim = c.g_dim; c.k.external = 1;
    c.comps.assign(s.comps, s.comps + s.n_comps);
    check_comps(c.comps, d->gd, "global constraint: global component out of range");
    c.jac0.assign(s.jac0, s.jac0 + (size_t)s.g_dim * s.n_comps);
    c.hess0.assign(s.hess0, s.hess0 + (size_t)s.n_comps * s.n_comps);
    c.n_times_total = 1;
    c.times0.push_back(d->N);
    return c;
}

ConHost knot_constraint(const dto_problem_desc* d, const dto_constraint_desc& s) {
    if (s.n_comps < 1 || !s.comps || (!s.times && s.n_times > 0)) throw HipError{"constraint: bad description"};
    ConHost c;
    c.k.kind = s.kind; c.k.n_comps = s.n_comps; c.k.c = s.c;
    c.equality = s.equality;
    if (s.kind == DTO_CONSTRAINT_EXTERNAL) {
        if (s.g_dim < 1) throw HipError{"external constraint: g_dim must be >= 1"};
        if (!s.jac0) throw HipError{"external constraint: jac0 (Jacobian blocks at Z0) is required for the sparsity pattern"};
        c.external = true;
        c.g_dim = s.g_dim;
        c.jac0.assign(s.jac0, s.jac0 + (size_t)s.g_dim * s.n_comps * s.n_times);
    } else if (s.g_dim > 1) {
        throw HipError{"constraint: the built-in kinds have g_dim = 1"};
    }
    c.k.g_dim = c.g_dim; c.k.external = c.external ? 1 : 0;
    c.comps.assign(s.comps, s.comps + s.n_comps);
    check_comps(c.comps, d->z, "constraint: component out of range");
    if (s.kind == DTO_CONSTRAINT_QUADFORM_MINUS_C) {
        if (!s.hess0) throw HipError{"quadratic-form constraint: the matrix M (hess0, n_comps x n_comps) is required"};
        const size_t n = (size_t)s.n_comps;
        std::vector<int32_t> sc = c.comps;
        std::sort(sc.begin(), sc.end());
        if (std::adjacent_find(sc.begin(), sc.end()) != sc.end())
            throw HipError{"quadratic-form constraint: a component is listed twice in comps"};
        c.M.assign(s.hess0, s.hess0 + n * n);
        for (size_t a = 0; a < n; ++a)
            for (size_t b2 = a + 1; b2 < n; ++b2)
                if (!(c.M[a + n * b2] == c.M[b2 + n * a])) throw HipError{"quadratic-form constraint: M is not symmetric"};
    }
    c.n_times_total = s.n_times;
    for (int64_t t = 0; t < s.n_times; ++t) c.times0.push_back(knot0(s.times[t], d->N, "constraint"));
    return c;
}

// nonlinear knot constraints: rows follow the dynamics (evaluator.jl:219-223); slots follow the external integrators'
void add_constraints(dto_handle* h, const dto_problem_desc* d) {
    int64_t row = h->n_dyn;
    for (int i = 0; i < d->n_constraints; ++i) {
        const dto_constraint_desc& s = d->constraints[i];
        if (s.kind != DTO_CONSTRAINT_NORM_MINUS_C && s.kind != DTO_CONSTRAINT_SQNORM_MINUS_C && s.kind != DTO_CONSTRAINT_EXTERNAL &&
            s.kind != DTO_CONSTRAINT_EXTERNAL_GLOBAL && s.kind != DTO_CONSTRAINT_QUADFORM_MINUS_C)
            throw HipError{"unknown constraint kind"};
        ConHost c = s.kind == DTO_CONSTRAINT_EXTERNAL_GLOBAL ? global_constraint(d, s) : knot_constraint(d, s);
        c.row_off = row;
        row += c.n_times_total * c.g_dim;
        h->con.push_back(std::move(c));
    }
    h->n_cons = row;
    for (auto& c : h->con)
        if (c.external) {
            c.ext_slot = (int)h->ext.size();
            ExtSlot e;
            e.len[0] = (size_t)c.g_dim * c.n_times_total;
            e.len[1] = (size_t)c.g_dim * c.comps.size() * c.n_times_total;
            e.len[2] = c.comps.size() * c.comps.size() * (size_t)c.n_times_total;
            h->ext.push_back(e);
        }
    h->n_ext_con = (int)h->ext.size() - h->n_ext_int;
}

// host-evaluated objective terms: their slots follow the constraints', and the Global* ones shape the Hessian structure
void add_external_objectives(dto_handle* h, const dto_problem_desc* d) {
    for (int i = 0; i < d->n_objectives; ++i) {
        const dto_objective_desc& s = d->objectives[i];
        if (s.kind != DTO_OBJECTIVE_EXTERNAL_KNOT && s.kind != DTO_OBJECTIVE_EXTERNAL_GLOBAL) continue;
        ExtObjHost e;
        e.weight = s.weight;
        e.global = s.kind == DTO_OBJECTIVE_EXTERNAL_GLOBAL;
        if (s.n_comps > 0) {
            if (!s.comps) throw HipError{"external objective: comps is null"};
            e.comps.assign(s.comps, s.comps + s.n_comps);
        }
        check_comps(e.comps, d->z, "external objective: component out of range");
        if (e.global) {
            if (s.n_gcomps < 1 || !s.gcomps) throw HipError{"global objective: gcomps are required"};
            e.gcomps.assign(s.gcomps, s.gcomps + s.n_gcomps);
            check_comps(e.gcomps, d->gd, "global objective: global component out of range");
        } else if (e.comps.empty() || !s.times) {
            throw HipError{"external knot objective: comps and times are required"};
        }
        if (s.n_times > 0 && !s.times) throw HipError{"external objective: times is null"};
        for (int64_t t = 0; t < s.n_times; ++t) e.times0.push_back(knot0(s.times[t], d->N, "objective"));
        if (e.times0.empty()) {  // GlobalObjective: the global variables alone
            if (!e.comps.empty()) throw HipError{"global objective: knot components without times"};
            e.times0.push_back(d->N);
        }
        const size_t nb = e.comps.size() + e.gcomps.size(), nl = e.times0.size();
        e.ext_slot = (int)h->ext.size();
        ExtSlot sl;
        sl.len[0] = nl; sl.len[1] = nb * nl; sl.len[2] = nb * nb * nl;
        h->ext.push_back(sl);
        h->ext_obj.push_back(std::move(e));
    }
    h->n_ext_obj = (int)h->ext_obj.size();
}

// ---- this handle's shard

// the listings of constraint c at owned knots: their local rows (from lrow on) and their places in the Jacobian slab
void place_constraint(dto_handle* h, ConHost& c, int64_t& lrow) {
    std::vector<int64_t> times, lrows, tidx, jpos;
    std::vector<int32_t> hess_on;
    for (int64_t i = 0; i < c.n_times_total; ++i) {
        const int64_t kn = c.times0[i];
        if (kn >= h->N ? h->k_hi != h->N : !owns_knot(h, kn)) continue;  // pseudo-knot N: last rank
        times.push_back(kn);
        lrows.push_back(lrow);
        lrow += c.g_dim;
        tidx.push_back(i);
        hess_on.push_back(last_listing_of_knot(c.times0.data(), c.n_times_total, i) ? 1 : 0);
        for (size_t q = 0; q < c.comps.size(); ++q) {
            const int64_t col = kn * h->z + c.comps[q];
            const size_t lo = con_lower(h, col);
            for (int r = 0; r < c.g_dim; ++r) {
                int64_t pos = -1;
                for (size_t e = lo; e < h->con_cols.size() && h->con_cols[e] == col; ++e)
                    if (h->con_rows[e] == c.row_off + i * c.g_dim + r) {
                        pos = con_entry_pos(h, col, (int64_t)(e - lo));
                        break;
                    }
                jpos.push_back(pos);
            }
        }
    }
    c.k.n_times = (int64_t)times.size();
    c.k.mu_off = c.row_off;
    {
        std::vector<int64_t> st = times;
        std::sort(st.begin(), st.end());
        c.k.repeats = std::adjacent_find(st.begin(), st.end()) != st.end() ? 1 : 0;
        std::vector<int32_t> sc = c.comps;
        std::sort(sc.begin(), sc.end());
        c.k.comp_repeats = std::adjacent_find(sc.begin(), sc.end()) != sc.end() ? 1 : 0;
    }
    if (h->structure_only) return;
    c.k.comps = own(h, dupload(c.comps));
    c.k.times = own(h, dupload(times));
    c.k.lrow = own(h, dupload(lrows));
    c.k.tidx = own(h, dupload(tidx));
    c.k.hess_on = own(h, dupload(hess_on));
    c.k.jpos = own(h, dupload(jpos));
    if (!c.M.empty()) c.k.M = own(h, dupload(c.M));
    if (c.external) {  // Hessian blocks: knot constraints place knot entries, the global one tail entries
        c.xk.nc = c.global ? 0 : (int32_t)c.comps.size();
        c.xk.ng = c.global ? (int32_t)c.comps.size() : 0;
        c.xk.comps = c.k.comps; c.xk.gcomps = c.k.comps;
        c.xk.times = c.k.times; c.xk.tidx = c.k.tidx;
        c.xk.knot_on = c.k.hess_on; c.xk.count = c.k.hess_on;
        c.xk.glob_on = h->k_hi == h->N ? 1 : 0;
        c.xk.n_list = c.k.n_times;
    }
}

// the sparsity structure, this handle's extents inside the global vectors, and its local constraint rows: integrators first,
// then constraints
void layout_shard(dto_handle* h, const dto_problem_desc* d) {
    const bool sonly = h->structure_only;
    KProb& P = h->P;
    P.N = h->N; P.K = h->K; P.z = h->z; P.dt_idx = h->dt_idx; P.D = h->D;
    P.kn_lo = h->k_lo - 1;
    P.n_knots = h->k_hi - h->k_lo + 1;
    P.n_int = std::max<int64_t>(0, std::min<int64_t>(h->k_hi, h->K) - h->k_lo + 1);

    build_structure(h, d->Z0);
    if (!sonly) {
        h->d_colptr = own(h, dupload(h->colptr));
        P.colptr = h->d_colptr;
    }
    const ShardExtents ext = shard_extents(h, h->k_lo, h->k_hi);
    P.jac_lo = ext.jac_lo;
    P.hess_lo = ext.hess_lo;
    P.grad_lo = ext.grad_lo;
    dto_shard_info& I = h->info;
    I.k_lo = h->k_lo; I.k_hi = h->k_hi;
    I.n_vars = h->n_vars; I.n_cons = h->n_cons; I.jac_nnz = h->jac_nnz; I.hess_nnz = h->hess_nnz;
    I.grad_lo = ext.grad_lo; I.grad_len = ext.grad_len;
    I.jac_lo = ext.jac_lo; I.jac_len = ext.jac_len;      // global columns ride with the last knot
    I.hess_lo = ext.hess_lo; I.hess_len = ext.hess_len;
    P.tail_lo = h->k_hi == h->N ? h->hess_block_nnz - P.hess_lo : -1;
    if (!sonly) {
        P.tail_colptr = own(h, dupload(h->tail_colptr));
        P.tail_rows = own(h, dupload(h->tail_rows));
    }

    int64_t lrow = 0;
    for (size_t i = 0; i < h->integ_kind.size(); ++i) {
        const int dd = h->integ_dim[i];
        if (h->integ_kind[i] == DTO_INTEGRATOR_BILINEAR) h->bil[h->integ_index[i]].k.lrow_off = lrow;
        else if (h->integ_kind[i] == DTO_INTEGRATOR_DERIVATIVE) h->der[h->integ_index[i]].lrow_off = lrow;
        else if (h->integ_kind[i] == DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR) h->tdb[h->integ_index[i]].place.lrow_off = lrow;
        else h->ext_int[h->integ_index[i]].lrow_off = lrow;
        lrow += P.n_int * dd;
    }
    for (auto& c : h->con) place_constraint(h, c, lrow);
    h->row_segments = shard_row_segments(h, h->k_lo, h->k_hi);  // the local buffer is their concatenation, in this order
    h->cons_len = lrow;
    I.cons_len = lrow;
    I.n_row_segments = (int32_t)h->row_segments.size();
}

// stable order of the listings by layer (occurrence index of their knot): returns the permutation, fills layer_start
std::vector<size_t> layer_order(const std::vector<int64_t>& t, std::vector<int64_t>& layer_start) {
    std::map<int64_t, int> seen;
    std::vector<int> layer(t.size());
    int nl = 0;
    for (size_t q = 0; q < t.size(); ++q) { layer[q] = seen[t[q]]++; nl = std::max(nl, layer[q] + 1); }
    std::vector<size_t> perm(t.size());
    for (size_t q = 0; q < perm.size(); ++q) perm[q] = q;
    std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b2) { return layer[a] < layer[b2]; });
    layer_start.assign((size_t)nl + 1, 0);
    for (size_t q = 0; q < t.size(); ++q) layer_start[(size_t)layer[q] + 1]++;
    for (int l = 0; l < nl; ++l) layer_start[(size_t)l + 1] += layer_start[(size_t)l];
    if (t.empty()) layer_start.assign(1, 0);
    return perm;
}

template <class V>
void permute(V& v, const std::vector<size_t>& perm, size_t width) {
    if (v.empty()) return;
    auto src = v;
    for (size_t q = 0; q < perm.size(); ++q)
        for (size_t c = 0; c < width; ++c) v[q * width + c] = src[perm[q] * width + c];
}

// the built-in objective terms at owned knots.  They exist on the device only: a structure-only handle skips the stage, and
// with it the checks of their descriptions.
void place_objectives(dto_handle* h, const dto_problem_desc* d) {
    const KProb& P = h->P;
    for (int i = 0; i < d->n_objectives; ++i) {
        const dto_objective_desc& s = d->objectives[i];
        KObj o{};
        o.kind = s.kind; o.weight = s.weight; o.D = s.D;
        std::vector<int64_t> times;
        std::vector<int64_t> layer_start;
        if (s.kind == DTO_OBJECTIVE_MINIMUM_TIME) {
            for (int64_t kn = P.kn_lo; kn < P.kn_lo + P.n_knots; ++kn)
                if (kn < h->K) times.push_back(kn);
            (void)layer_order(times, layer_start);
        } else if (s.kind == DTO_OBJECTIVE_QUADRATIC_REGULARIZER || s.kind == DTO_OBJECTIVE_LINEAR_REGULARIZER) {
            if (s.comp_dim < 1 || s.comp_off < 0 || s.comp_off + s.comp_dim > d->z || !s.R)
                throw HipError{"objective: bad component range"};
            o.comp_off = s.comp_off; o.comp_dim = s.comp_dim;
            o.R = own(h, dupload(std::vector<double>(s.R, s.R + s.comp_dim)));
            if (s.baseline && s.kind == DTO_OBJECTIVE_QUADRATIC_REGULARIZER) {
                o.has_baseline = 1;
                o.baseline = own(h, dupload(std::vector<double>(s.baseline, s.baseline + (size_t)s.comp_dim * d->N)));
            }
            if (s.times) {
                for (int64_t t = 0; t < s.n_times; ++t) {
                    const int64_t kn = knot0(s.times[t], d->N, "objective");
                    if (owns_knot(h, kn)) times.push_back(kn);
                }
            } else {
                for (int64_t kn = P.kn_lo; kn < P.kn_lo + P.n_knots; ++kn) times.push_back(kn);
            }
            permute(times, layer_order(times, layer_start), 1);
        } else if (s.kind == DTO_OBJECTIVE_KNOT_SQDIST || s.kind == DTO_OBJECTIVE_KNOT_LOWRANK_INFIDELITY) {
            if (s.n_comps < 1 || !s.comps || !s.times) throw HipError{"knot objective: comps and times are required"};
            if (s.kind == DTO_OBJECTIVE_KNOT_LOWRANK_INFIDELITY) {
                if (s.comp_dim < 1 || !s.R) throw HipError{"low-rank infidelity: the factor A (R) and its row count (comp_dim) are required"};
                o.comp_dim = s.comp_dim;
                o.R = own(h, dupload(std::vector<double>(s.R, s.R + (size_t)s.comp_dim * s.n_comps)));
            }
            std::vector<int32_t> comps(s.comps, s.comps + s.n_comps);
            check_comps(comps, d->z, "knot objective: component out of range");
            std::vector<double> params, Qs;
            std::vector<int32_t> last;
            for (int64_t t = 0; t < s.n_times; ++t) {
                const int64_t kn = knot0(s.times[t], d->N, "objective");
                if (!owns_knot(h, kn)) continue;
                times.push_back(kn);
                Qs.push_back(s.Qs ? s.Qs[t] : 1.0);
                if (s.params) params.insert(params.end(), s.params + (size_t)t * s.n_comps, s.params + (size_t)(t + 1) * s.n_comps);
                last.push_back(last_listing_of_knot(s.times, s.n_times, t) ? 1 : 0);
            }
            {
                const std::vector<size_t> perm = layer_order(times, layer_start);
                permute(times, perm, 1);
                permute(Qs, perm, 1);
                permute(last, perm, 1);
                permute(params, perm, (size_t)s.n_comps);
            }
            o.n_comps = s.n_comps;
            o.comps = own(h, dupload(comps));
            o.Qs = own(h, dupload(Qs));
            o.last = own(h, dupload(last));
            o.params = s.params ? own(h, dupload(params)) : nullptr;
        } else if (s.kind == DTO_OBJECTIVE_EXTERNAL_KNOT || s.kind == DTO_OBJECTIVE_EXTERNAL_GLOBAL) {
            continue;  // placed by the external-term kernels (place_external_objectives)
        } else {
            throw HipError{"unknown objective kind"};
        }
        o.n_times = (int64_t)times.size();
        o.times = own(h, dupload(times));
        h->obj.push_back(o);
        dto_handle::ObjInfo oi;
        oi.layer_start = layer_start;
        oi.kind = s.kind; oi.comp_off = s.comp_off; oi.comp_dim = s.comp_dim; oi.times = times;
        if (s.comps && s.n_comps > 0) oi.comps.assign(s.comps, s.comps + s.n_comps);
        h->obj_info.push_back(std::move(oi));
    }
}

// host-evaluated objective terms: which listings this handle places (knot part: the knot's owner; entries in
// global-variable columns and listings without a knot part: the rank that owns the last knot)
void place_external_objectives(dto_handle* h) {
    const bool last_rank = h->k_hi == h->N;
    for (auto& e : h->ext_obj) {
        std::vector<int64_t> times, tix;
        std::vector<int32_t> knot_on, count;
        for (size_t i = 0; i < e.times0.size(); ++i) {
            const int64_t kn = e.times0[i];
            const bool pseudo = kn >= h->N;
            const bool own = pseudo ? last_rank : owns_knot(h, kn);
            if (!own && !(e.global && last_rank)) continue;
            int32_t on = own && !pseudo;
            // KnotPointObjective's gradient!/hessian! overwrite per listing: the last one wins
            if (on && !e.global && !last_listing_of_knot(e.times0.data(), (int64_t)e.times0.size(), (int64_t)i)) on = 0;
            times.push_back(kn);
            tix.push_back((int64_t)i);
            knot_on.push_back(on);
            count.push_back(own ? 1 : 0);
        }
        e.k.nc = (int32_t)e.comps.size(); e.k.ng = (int32_t)e.gcomps.size();
        e.k.n_list = (int64_t)times.size();
        e.k.glob_on = last_rank ? 1 : 0;
        if (h->structure_only) continue;
        e.k.comps = own(h, dupload(e.comps));
        e.k.gcomps = own(h, dupload(e.gcomps));
        e.k.times = own(h, dupload(times));
        e.k.tidx = own(h, dupload(tix));
        e.k.knot_on = own(h, dupload(knot_on));
        e.k.count = own(h, dupload(count));
    }
}

// ---- device workspaces (not reached by a structure-only handle)

void alloc_scratch(dto_handle* h) {
    h->d_Z = own(h, dalloc<double>(h->n_vars));
    h->d_mu = own(h, dalloc<double>(std::max<int64_t>(h->n_cons, 1)));
    h->d_partial = own(h, dalloc<double>(256));
    h->d_f = own(h, dalloc<double>(1));
    h->d_bounds = own(h, dalloc<double>(2));
    h->d_plan = own(h, dalloc<int32_t>(4));
    HIP_CHECK(hipHostMalloc((void**)&h->mailbox, sizeof(PinnedMailbox)));
    HIP_CHECK(hipHostMalloc((void**)&h->h_stats, sizeof(int32_t) * 4 * std::max<size_t>(h->bil.size(), 1)));
    memset(h->h_stats, 0, sizeof(int32_t) * 4 * std::max<size_t>(h->bil.size(), 1));
}

// device buffers of the time-dependent bilinear integrators: blocks indexed by the global interval (like the host-evaluated
// integrators' arrays), one scratch slab per interval this handle evaluates
void alloc_tdb(dto_handle* h) {
    const bool hess = h->eval_hessian != 0;
    for (auto& t : h->tdb) {
        const size_t n = t.k.n, z = h->z, K = (size_t)h->K;
        t.d_vals = own(h, dalloc<double>(K * n));
        t.d_jac = own(h, dalloc<double>(K * n * 2 * z));
        if (hess) t.d_hess = own(h, dalloc<double>(K * 4 * z * z));
        // the product modes (need 3, 4) share the scratch below with the value calls; their J' w stages n + p doubles per interval
        const int p = tdb_num_params(t.k.m, t.k.order);
        t.d_jtv = own(h, dalloc<double>(std::max<size_t>(K, 1) * (n + (size_t)p)));
        if (t.kron) {
            // the kernel assigns the entries it owns and nothing else: the constant zeros of the blocks are written here, once
            HIP_CHECK(hipMemset(t.d_jac, 0, K * n * 2 * z * sizeof(double)));
            if (hess) HIP_CHECK(hipMemset(t.d_hess, 0, K * 4 * z * z * sizeof(double)));
            t.resident = (int)std::min<int64_t>(h->P.n_knots + 1, 2 * (int64_t)std::max(h->n_cu, 1));
            t.stride = scratch_stride(std::max({tdb_kron_scratch_doubles(t.k, t.kk, 1), tdb_kron_scratch_doubles(t.k, t.kk, 3),
                                                tdb_kron_scratch_doubles(t.k, t.kk, 4)}),
                                      tdb_kron_scratch_doubles(t.k, t.kk, 2), hess);
            t.d_scratch = own(h, dalloc<double>(t.stride * (size_t)t.resident));
            continue;
        }
        if (t.mfma) {
            // sized by the persistent grid (two workgroups per compute unit), not by the number of intervals
            t.resident = (int)std::min<int64_t>(h->P.n_knots + 1, 2 * (int64_t)std::max(h->n_cu, 1));
            t.stride = scratch_stride(std::max({tdb_mfma_scratch_doubles(t.k, 1), tdb_mfma_scratch_doubles(t.k, 3), tdb_mfma_scratch_doubles(t.k, 4)}),
                                      tdb_mfma_scratch_doubles(t.k, 2), hess);
            t.d_scratch = own(h, dalloc<double>(t.stride * (size_t)t.resident));
            if (!t.share_members.empty()) {   // leader of an active group: the slots of the group launches
                const int g = t.share_cap;
                t.share_stride = scratch_stride(std::max(tdb_mfma_scratch_doubles(t.k, 0, g), tdb_mfma_scratch_doubles(t.k, 1, g)),
                                                tdb_mfma_scratch_doubles(t.k, 2, g), hess);
                t.d_share_scratch = own(h, dalloc<double>(t.share_stride * (size_t)t.resident));
            }
            continue;
        }
        t.stride = scratch_stride(std::max({tdb_scratch_doubles(t.k, 1), tdb_scratch_doubles(t.k, 3), tdb_scratch_doubles(t.k, 4)}),
                                  tdb_scratch_doubles(t.k, 2), hess);
        t.d_scratch = own(h, dalloc<double>(t.stride * (size_t)(h->P.n_knots + 1)));
    }
}

// structured path: one term slab per owned interval; the statistics words sit where the sweeps' do (deferred error convention)
void alloc_kron(dto_handle* h, BilHost& b) {
    // (the product modes' r-column pw / pa group takes more room than the Jacobian's b-column e group when r pads wider than b)
    b.kron_stride = scratch_stride(std::max(kron_scratch_doubles(b.kk, b.k.m, 1), kron_scratch_doubles(b.kk, b.k.m, 3)),
                                   kron_scratch_doubles(b.kk, b.k.m, 2), h->eval_hessian != 0);
    b.d_kron_scratch = own(h, dalloc<double>(b.kron_stride * (size_t)std::max<int64_t>(h->P.n_int, 1)));
    b.kk.stats = own(h, dalloc<int32_t>(2));
    HIP_CHECK(hipMemset(b.kk.stats, 0, 2 * sizeof(int32_t)));
    b.fw.stats = b.kk.stats;
}

// Hessian pairing path: term stores for both sweeps + E_j*terms + Beta-weighted sums (skipped when they would take more than
// 40 % of the free HBM: the second-order sweep is then used)
// (80 terms: the step budget from the cheap norm bound of the 256 x 2000 benchmark is 66 -- with 64 the Hessian bought the exact
// norms, a store-less basis GEMM and two round trips, only to fit its budget into the store)
void alloc_pairing_store(dto_handle* h, BilHost& b) {
    const int m = b.k.m, dcap = PAIR_DCAP, T1 = 1 + m;
    const double bytes = (double)dcap * T1 * b.fw.Kpad * b.k.npad * 8.0;
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (!(m >= 1 && bytes * (3.0 + 1.0 * m / T1) < 0.4 * (double)free_b)) return;
    const size_t store = (size_t)dcap * T1 * b.fw.Kpad * b.k.npad;
    for (SweepBuf* w : {&b.fw, &b.ad}) {
        w->Zt = own(h, dalloc<double>(store));
        w->dcap = dcap;
        // one entry per convergence block; the fused sweep's blocks are as small as one interval
        w->nterms = own(h, dalloc<int32_t>(w->Kpad));
        HIP_CHECK(hipMemset(w->nterms, 0, sizeof(int32_t) * w->Kpad));
        w->nterms_p = own(h, dalloc<int32_t>(w->Kpad));
        HIP_CHECK(hipMemset(w->nterms_p, 0, sizeof(int32_t) * w->Kpad));
    }
    b.EP = own(h, dalloc<double>((size_t)m * dcap * b.fw.Kpad * b.k.npad));  // G_j' U_a
    b.Upair = own(h, dalloc<double>(store));
    std::vector<double> bt(PAIR_DCAP * PAIR_DCAP);
    for (int a = 0; a < PAIR_DCAP; ++a)
        for (int c = 0; c < PAIR_DCAP; ++c)
            bt[a * PAIR_DCAP + c] = std::exp(std::lgamma(a + 1.0) + std::lgamma(c + 1.0) - std::lgamma(a + c + 2.0));
    b.d_Btab = own(h, dupload(bt));
    b.pairing = true;
}

// N2[i][j] = ||G_i G_j||_1 with the engine's own batched GEMM + norm kernels, for the step-budget bounds
void generator_product_norms(dto_handle* h, BilHost& b) {
    const int npad = b.k.npad, m1 = b.k.m + 1, nb = m1 * m1;
    const size_t nn = (size_t)npad * npad;
    for (int i = 0; i < m1; ++i)
        for (int j = 0; j < m1; ++j) {
            HIP_CHECK(hipMemcpyAsync(b.chain.W[0] + (size_t)(i * m1 + j) * nn, b.k.G + (size_t)i * nn, nn * 8, hipMemcpyDeviceToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(b.chain.W[2] + (size_t)(i * m1 + j) * nn, b.k.G + (size_t)j * nn, nn * 8, hipMemcpyDeviceToDevice, h->stream));
        }
    launch_bgemm_plain(h->stream, npad, nb, b.chain.W[0], b.chain.W[2], b.chain.W[1]);
    launch_norm1(h->stream, npad, nb, b.chain);
    std::vector<double> norms((size_t)nb * 4);
    HIP_CHECK(hipMemcpyAsync(norms.data(), b.chain.norms, norms.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    b.n2.resize(nb);
    for (int i = 0; i < nb; ++i) b.n2[i] = norms[(size_t)i * 4 + 1];
    b.d_g1 = own(h, dupload(b.g1));
    b.d_n2 = own(h, dupload(b.n2));
}

// generator-subspace powers pay off while the number of symmetrised products stays well below the 3n columns the three GEMMs
// would process
bool basis_pays_off(const BilHost& b) {
    const long m1 = b.k.m + 1;
    const long c2 = m1 * (m1 + 1) / 2, c3 = c2 * (m1 + 2) / 3, c4 = c3 * (m1 + 3) / 4;
    // (npad is a multiple of 64: npad^2 is a multiple of the kernel's 128-row tiles and every wave's 64 rows of
    // vec(A^r) stay inside one matrix column, which is all k_basis_gemm's fused column sums need)
    return (c2 + c3 + c4) * 2 <= 3L * b.k.npad;
}

// per-bilinear workspaces + generator product norms
void alloc_bilinear(dto_handle* h) {
    const bool hess = h->eval_hessian != 0;
    for (auto& b : h->bil) {
        const int m = b.k.m;
        if (b.small) {
            if (hess && 1 + m + m * (m + 1) / 2 > MAX_TYPES) throw HipError{"bilinear integrator: too many drives for second-order sweep"};
            continue;  // the fused kernel needs no workspace
        }
        if (b.kron) {
            alloc_kron(h, b);
            continue;
        }
        const int T_fw = std::max(2 + m, hess ? 1 + m + m * (m + 1) / 2 : 1 + m);  // +1: exp(A)w_x column of J w
        if (T_fw > MAX_TYPES) throw HipError{"bilinear integrator: too many drives for the second-order sweep"};
        alloc_sweep(h, b, b.fw, T_fw, hess);  // W: G_l x for the Hessian's scalar blocks
        if (hess) {
            alloc_sweep(h, b, b.ad, 1 + m, true);
            alloc_pairing_store(h, b);
        }
        alloc_chain(h, b, std::max(chunk_size(h, b.k.npad), (m + 1) * (m + 1)));
        generator_product_norms(h, b);
        if (basis_pays_off(b)) build_basis(h, b, b.chain_cap);
    }
}

}  // namespace

extern "C" int dto_create(const dto_problem_desc* d, dto_handle** out) {
    if (!d || !out) return fail(nullptr, "dto_create: null argument");
    *out = nullptr;
    if (const char* why = check_desc(d)) return fail(nullptr, why);
    const bool sonly = d->device < 0;  // structure-only handle: no GPU is touched, evaluations fail
    std::unique_ptr<dto_handle> h(new dto_handle());
    try {
        h->device = d->device;
        h->structure_only = sonly;
        if (!sonly) open_device(h.get());
        set_dimensions(h.get(), d);
        add_integrators(h.get(), d);
        find_share_groups(h.get(), d);
        find_time_dependent_share_groups(h.get(), d);
        if (h->integ_kind.size() > 8) throw HipError{"at most 8 integrators"};
        add_constraints(h.get(), d);
        add_external_objectives(h.get(), d);
        layout_shard(h.get(), d);
        // (the stages up to here upload what they lay out as they go, and the two below keep their order: device allocations
        // happen in the same sequence as ever, which the pairing store's look at the free memory depends on)
        if (!sonly) place_objectives(h.get(), d);
        place_external_objectives(h.get());
        if (!sonly) {
            alloc_scratch(h.get());
            alloc_tdb(h.get());
            alloc_bilinear(h.get());
            HIP_CHECK(hipDeviceSynchronize());
        }
    } catch (const HipError& e) {
        return fail(nullptr, e.msg);
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
    *out = h.release();
    return 0;
}
