// dto_bgemm_dispatch.h -- which of the two batched FP64 GEMM kernels of dto_kernels.hip one launch runs on (nbatch products of
// npad x npad matrices, npad a multiple of 64), with its block size and grid.  Plain C++ (no HIP header, no engine header):
// launch_bgemm asks and launches, tests/test_bgemm_dispatch_header.py builds the rule with g++ alone.
//   tile64: k_bgemm<GemmShape<64,64,2,2,16>>, 256 threads, 64x64 tiles, operands staged through registers (dto_gemm.hip.h)
//   ring:   k_bgemm_r<.,4>, 512 threads, 128x128 tiles, K panels in an LDS ring by LDS-DMA (dto_gemm_ring.hip.h)
// Both kernels walk the list of batch_tile_count(nbatch, tiles per matrix) (interval, tile) slots with a stride of their grid.
#pragma once

namespace dto {

struct BGemmLaunch {
    bool ring;     // false: tile64
    int threads;
    int grid;
};

//   poly              the epilogue streams the stage polynomial's matrices (EPI_HORNER / EPI_DUAL / EPI_DUAL5)
//   force_tile64      DTO_BGEMM_TILE64: -1 the rule below, 0 / 1 forced wherever the ring kernel can run (TUNING builds)
//   ring_persist_all  DTO_BGEMM_RING = 1: the polynomial products persistent as well (TUNING builds)
inline BGemmLaunch bgemm_dispatch(int npad, int nbatch, bool poly, int force_tile64 = -1, bool ring_persist_all = false) {
    // The ring kernel needs whole 128-tiles.  It wins at every launch size from two tiles per side on (256 states x 30 intervals
    // included); with ONE tile per matrix a short launch is better served by four times as many 64x64 workgroups, and the measured
    // crossover is 3500 intervals.
    const bool small_launch = force_tile64 >= 0 ? force_tile64 != 0 : (npad == 128 && nbatch < 3500);
    const bool ring = npad % 128 == 0 && !small_launch;
    const int tiles_side = npad / (ring ? 128 : 64);
    int grid = (nbatch + 7) / 8 * 8 * tiles_side * tiles_side;   // batch_tile_count: one workgroup per slot ...
    // ... unless PERSISTENT, the grid sized to the chip's 256 CUs (tile64 4 workgroups per CU, ring 2): the plain products and the
    // squarings.  The polynomial products, bound by the bytes of their epilogues, keep one workgroup per tile (persistent they lose
    // 5-15 %).
    const int chip = ring ? 2 * 256 : 4 * 256;
    if ((!poly || (ring && ring_persist_all)) && grid > chip) grid = chip;
    return {ring, ring ? 512 : 256, grid};
}

}  // namespace dto
