// dto_quadform.hip -- NonlinearKnotPointConstraint with the built-in g(v) = [ v' M v - c ], M a constant symmetric
// n_comps x n_comps matrix (DTO_CONSTRAINT_QUADFORM_MINUS_C): final-fidelity bounds ||A v||^2 >= F_min (M = -A'A, c = -F_min),
// expectation values, weighted populations.
//
// Everything rests on y = M v of one listing, worked by a workgroup: lane c owns row c and walks j = 0 .. n_comps-1 in ascending
// order over M[c + n_comps j] -- column j of the column-major matrix, which symmetry makes row c's entries, so adjacent lanes read
// adjacent addresses -- against v staged in LDS.  The order (and the unfused multiply-add) is that of the host's pattern
// arithmetic at Z0 (dto_engine.cpp, con_jac_value).  LDS holds min(n_comps, QF_TILE) entries of v; a longer v passes through in
// tiles, j still ascending.
//
//   g, J w     one workgroup per listing: its threads take the rows c = t, t + 256, ... in order, then a fixed tree over the
//              256 partial sums (wavefront butterfly, four wavefront sums added in order) -- no atomics
//   J, J' w    one workgroup per (listing, tile of 256 rows): entry 2 y_c goes to jpos (dropped outside the Z0 pattern); J' w
//              adds 2 y_c w_row to its (knot, component) entry, and a constraint whose `times` repeat a knot walks its listings
//              in order inside the workgroup of each row tile, so every entry keeps one writer and a fixed order
//   Hessian    one thread per (listing, a, b), adjacent lanes on adjacent a: 2 mu_i M[a, b] on row <= col by component index,
//              exact zeros of M skipped, a single add into the zero-filled slab as k_hess_knot does; a knot listed twice
//              keeps the later listing's block (hess_on)
//
// Results depend on the listing's data alone: not on the grid, the shard or earlier calls.
#include "dto_kernels.h"

namespace dto {
namespace {

constexpr int QF_THREADS = 256;
constexpr int QF_TILE = 4096;  // entries of v in LDS at a time (32 KB)
constexpr int QF_AHEAD = 32;   // entries of a row of M loaded ahead of the sum (same order of addition)

__device__ __forceinline__ double qf_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double qf_block_sum(double v, double* sm) {
    v = qf_wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return sm[0] + sm[1] + sm[2] + sm[3];
}

// y_c = sum_j M[c + n j] v_j for the calling thread's row c (c >= n: no row, the thread only helps staging v); all threads of
// the workgroup call it together.  sv: min(n, QF_TILE) doubles of LDS.
__device__ __forceinline__ double qf_row(const KCon& C, const double* __restrict__ zk, int c, double* sv) {
    const int n = C.n_comps;
    double y = 0.0;
    for (int j0 = 0; j0 < n; j0 += QF_TILE) {
        const int jn = n - j0 < QF_TILE ? n - j0 : QF_TILE;
        __syncthreads();  // the tile before (or the listing before) has been consumed
        for (int j = threadIdx.x; j < jn; j += QF_THREADS) sv[j] = zk[C.comps[j0 + j]];
        __syncthreads();
        if (c < n) {
            const double* m = C.M + c + (int64_t)n * j0;
            {
#pragma clang fp contract(off)
                // the walk is one dependent chain per lane: QF_AHEAD loads of M are in flight before their products join it
                int j = 0;
                for (; j + QF_AHEAD <= jn; j += QF_AHEAD) {
                    double mv[QF_AHEAD];
#pragma unroll
                    for (int u = 0; u < QF_AHEAD; ++u) mv[u] = m[(int64_t)n * (j + u)];
#pragma unroll
                    for (int u = 0; u < QF_AHEAD; ++u) y = y + mv[u] * sv[j + u];
                }
                for (; j < jn; ++j) y = y + m[(int64_t)n * j] * sv[j];
            }
        }
    }
    return y;
}

// JW = 0: g[lrow] = v' (M v) - c;  JW = 1: y[row] += sum_c 2 (M v)_c w_c over the entries inside the pattern
template <int JW>
__global__ void __launch_bounds__(QF_THREADS) k_qf_reduce(KProb P, KCon C, const double* __restrict__ Z, const double* __restrict__ w,
                                                           double* __restrict__ out) {
    extern __shared__ double sv[];
    __shared__ double sm[4];
    const int64_t ti = blockIdx.x;
    const int64_t kn = C.times[ti];
    const double* zk = Z + kn * P.z;
    const int n = C.n_comps;
    double acc = 0.0;
    int any = 0;
    for (int c0 = 0; c0 < n; c0 += QF_THREADS) {
        const int c = c0 + (int)threadIdx.x;
        const double y = qf_row(C, zk, c, sv);
        if (c < n) {
            if (JW) {
                if (C.jpos[ti * n + c] >= 0) {
                    acc += 2.0 * y * w[kn * P.z + C.comps[c]];
                    any = 1;
                }
            } else {
                acc += zk[C.comps[c]] * y;
            }
        }
    }
    if (JW) any = __syncthreads_or(any);
    const double s = qf_block_sum(acc, sm);
    if (threadIdx.x != 0) return;
    if (JW) {
        if (any) out[C.mu_off + C.tidx[ti]] += s;
    } else {
        out[C.lrow[ti]] = s - C.c;
    }
}

// JTW = 0: vals[jpos] = 2 (M v)_c;  JTW = 1: y[knot, comp_c] += 2 (M v)_c w[row].  blockIdx.x = listing * tiles + row tile, or
// (serial) the row tile alone, the listings walked in order.
template <int JTW>
__global__ void __launch_bounds__(QF_THREADS) k_qf_entries(KProb P, KCon C, const double* __restrict__ Z, const double* __restrict__ w,
                                                            double* __restrict__ out, int tiles, int serial) {
    extern __shared__ double sv[];
    const int n = C.n_comps;
    const int64_t t0 = serial ? 0 : (int64_t)(blockIdx.x / (unsigned)tiles);
    const int64_t t1 = serial ? C.n_times : t0 + 1;
    const int c = (int)(blockIdx.x % (unsigned)tiles) * QF_THREADS + (int)threadIdx.x;
    for (int64_t ti = t0; ti < t1; ++ti) {
        const int64_t kn = C.times[ti];
        const double y = qf_row(C, Z + kn * P.z, c, sv);
        if (c >= n) continue;
        const int64_t p = C.jpos[ti * n + c];
        if (p < 0) continue;
        if (JTW) out[kn * P.z + C.comps[c]] += 2.0 * y * w[C.mu_off + C.tidx[ti]];
        else out[p] = 2.0 * y;
    }
}

__global__ void __launch_bounds__(QF_THREADS) k_qf_hess(KProb P, KCon C, const double* __restrict__ mu, double* __restrict__ H) {
    const int64_t i = (int64_t)blockIdx.x * QF_THREADS + threadIdx.x;
    const int64_t n = C.n_comps, nc2 = n * n;
    if (i >= C.n_times * nc2) return;
    const int64_t ti = i / nc2;
    if (!C.hess_on[ti]) return;
    const int64_t ab = i - ti * nc2;
    const int a = (int)(ab % n), b = (int)(ab / n);
    const int ca = C.comps[a], cb = C.comps[b];
    if (ca > cb) return;
    const double m = C.M[ab];
    if (m == 0.0) return;
    atomicAdd(&H[hess_pos(P, C.times[ti], ca, cb)], 2.0 * mu[C.mu_off + C.tidx[ti]] * m);
}

inline size_t qf_lds(const KCon& C) { return sizeof(double) * (size_t)(C.n_comps < QF_TILE ? C.n_comps : QF_TILE); }
inline int qf_tiles(const KCon& C) { return (C.n_comps + QF_THREADS - 1) / QF_THREADS; }

}  // namespace

void launch_qf_cons(hipStream_t st, const KProb& P, const KCon& C, const double* dZ, double* g) {
    if (C.n_times <= 0) return;
    hipLaunchKernelGGL(k_qf_reduce<0>, dim3((unsigned)C.n_times), dim3(QF_THREADS), qf_lds(C), st, P, C, dZ, nullptr, g);
}
void launch_qf_jac(hipStream_t st, const KProb& P, const KCon& C, const double* dZ, double* vals) {
    if (C.n_times <= 0) return;
    const int tiles = qf_tiles(C);
    hipLaunchKernelGGL(k_qf_entries<0>, dim3((unsigned)(C.n_times * tiles)), dim3(QF_THREADS), qf_lds(C), st, P, C, dZ, nullptr, vals,
                       tiles, 0);
}
void launch_qf_jv(hipStream_t st, const KProb& P, const KCon& C, const double* dZ, const double* w, double* y, int transpose) {
    if (C.n_times <= 0) return;
    if (!transpose) {
        hipLaunchKernelGGL(k_qf_reduce<1>, dim3((unsigned)C.n_times), dim3(QF_THREADS), qf_lds(C), st, P, C, dZ, w, y);
        return;
    }
    const int tiles = qf_tiles(C);
    const int serial = C.repeats ? 1 : 0;  // listings that repeat a knot meet in one entry: walked in listing order
    hipLaunchKernelGGL(k_qf_entries<1>, dim3((unsigned)(serial ? tiles : C.n_times * tiles)), dim3(QF_THREADS), qf_lds(C), st, P, C, dZ, w,
                       y, tiles, serial);
}
void launch_qf_hess(hipStream_t st, const KProb& P, const KCon& C, const double* dmu, double* H) {
    const int64_t n = C.n_times * C.n_comps * C.n_comps;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_qf_hess, dim3((unsigned)((n + QF_THREADS - 1) / QF_THREADS)), dim3(QF_THREADS), 0, st, P, C, dmu, H);
}

}  // namespace dto
