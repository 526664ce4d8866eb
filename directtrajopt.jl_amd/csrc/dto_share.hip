// dto_share.hip -- DTO_FLAG_SHARED_GENERATORS: bilinear integrators with equal generators, controls and timestep have the same
// propagators E_k = exp(dt_k G(u_k)); the chain runs for the group's leader alone and k_share_E copies its -E_k blocks to the
// followers' positions in the Jacobian slab.
//
// A block is n columns of n consecutive entries each; the columns lie a whole CSC column apart (other integrators' rows and the
// knot constraints' entries sit between them), so source and destinations are addressed column by column with the arithmetic of
// the chain's final store (jac_pos).  A wavefront takes one column: it reads the leader's run once into registers and writes
// it to every follower, whose address is formed once per column.  Runs start at any multiple of 8 bytes; each is split into an odd head entry, 16-byte pairs and an odd tail
// entry.  Where a follower's run has the other 16-byte phase than the leader's, the wavefront reads the leader's run a second
// time in that phase (two 8-byte loads per lane from lines the first read just brought in) so that its stores are 16 bytes
// wide as well.  Plain loads and stores: every destination entry has one writer, nothing is accumulated.
#include "dto_kernels.h"

namespace dto {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));

__device__ inline int phase_of(const double* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 3) & 1); }

__global__ void __launch_bounds__(256) k_share_E(KProb P, KShare S, int64_t int0, double* __restrict__ vals) {
    const int64_t kn = int0 + blockIdx.x;
    const int n = S.n;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int col = 4 * blockIdx.y + wave; col < n; col += 4 * gridDim.y) {
        const double* src = vals + jac_pos(P, P.colptr, kn, S.x_off[0] + col, S.pre[0], n, 1, 0);
        const int hs = phase_of(src);   // 1: the run starts with an odd entry
        const int ho = hs ^ 1;
        // which followers' runs have the other phase (the same for every lane of the wavefront)
        unsigned other = 0;
        for (int f = 1; f <= S.nf; ++f)
            other |= (unsigned)(phase_of(vals + jac_pos(P, P.colptr, kn, S.x_off[f] + col, S.pre[f], n, 1, 0)) != hs) << f;
        const int np_s = (n - hs) / 2, np_o = (n - ho) / 2;
        const double first = src[0], last = src[n - 1];
        // the run in pieces of up to SEG pairs per lane: read into registers once, then follower by follower -- a follower's
        // address (one load of its column pointer, the same for every lane) is formed once per piece, not once per store
        constexpr int SEG = 8;   // 8 x 64 pairs: a run of up to 1024 entries is one piece
        for (int i0 = 0; i0 < (n + 1) / 2; i0 += 64 * SEG) {
            d2 vs[SEG], vo[SEG];
#pragma unroll
            for (int q = 0; q < SEG; ++q) {
                const int i = i0 + 64 * q + lane;
                vs[q] = d2{0.0, 0.0};
                vo[q] = d2{0.0, 0.0};
                if (i < np_s) vs[q] = *reinterpret_cast<const d2*>(src + hs + 2 * i);
                if (other && i < np_o) { vo[q].x = src[ho + 2 * i]; vo[q].y = src[ho + 2 * i + 1]; }
            }
            for (int f = 1; f <= S.nf; ++f) {
                double* dst = vals + jac_pos(P, P.colptr, kn, S.x_off[f] + col, S.pre[f], n, 1, 0);
                const bool o = (other >> f) & 1u;
                const int hd = o ? ho : hs, np_d = o ? np_o : np_s;
#pragma unroll
                for (int q = 0; q < SEG; ++q) {
                    const int i = i0 + 64 * q + lane;
                    if (i < np_d) *reinterpret_cast<d2*>(dst + hd + 2 * i) = o ? vo[q] : vs[q];
                }
                if (i0 == 0 && lane == 0 && hd) dst[0] = first;
                if (i0 == 0 && lane == 0 && hd + 2 * np_d < n) dst[n - 1] = last;
            }
        }
    }
}

}  // namespace

void launch_share_E(hipStream_t st, const KProb& P, const KShare& S, int64_t int0, int nb, double* vals) {
    if (nb <= 0 || S.nf <= 0 || S.n <= 0) return;
    const int gy = S.n >= 256 ? 16 : (S.n + 15) / 16;   // at least four columns per wavefront
    hipLaunchKernelGGL(k_share_E, dim3((unsigned)nb, (unsigned)gy), dim3(P.debug_bad_launch ? 4096 : 256), 0, st, P, S, int0, vals);
}

}  // namespace dto
