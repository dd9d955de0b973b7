// The build parameters of the kernels: every macro a -D on the compiler's command line may override (tools/build_variant.sh),
// each a number of size, occupancy or tolerance.  Code variants are not here: an experiment that was decided is
// resolved in the source, with its figure at the code that won ("retired build switches").
// tests/test_build_switches.py holds the sources to this list.
#pragma once

// ---- tiled flux launch (eqlb_se_tile.h) ----
#ifndef EQLB_TILE_THREADS
#define EQLB_TILE_THREADS 512 // k <= 2: 8 waves per tile, two workgroups per CU
#endif
#ifndef EQLB_TILE_THREADS_K3
#define EQLB_TILE_THREADS_K3 512 // the k = 3 body runs at 2 waves/SIMD: ONE 8-wave workgroup per CU with the whole LDS
#endif
#ifndef EQLB_TILE_CELLS
#define EQLB_TILE_CELLS 480 // 480 cells x 18 packed values + tables: two workgroups per CU (SE and EV)
#endif
#ifndef EQLB_TILE_CELLS_K3
#define EQLB_TILE_CELLS_K3 492 // LARGEST tile: 492 cells x 36 packed values (141.7 KB) + 21.2 KB of tables (half of WQ) of the 160 KB: one workgroup per CU
#endif
#ifndef EQLB_TILE_CELLS_K3_EV
#define EQLB_TILE_CELLS_K3_EV 468 // EV mode stages 7.2 KB more tensors (HG, WG)
#endif
#ifndef EQLB_PAIR_LANES
#define EQLB_PAIR_LANES 1 // full 8-cell RT_2 patches on four lanes (eqlb_se_kernels_pair.hip); 0: the full-patch instance, 8 per wave-block, for every full patch (register report and A/B)
#endif

// ---- per-bin and fused flux launches (eqlb_se_launch.h) ----
#ifndef EQLB_K4_WAVES
#define EQLB_K4_WAVES 1 // waves per SIMD asked for the register-solver kernels at k = 4 (1: up to 512 registers)
#endif
#ifndef EQLB_FUSED_WAVES
#define EQLB_FUSED_WAVES 4 // waves per SIMD asked for k_se_patch_fused at k <= 2
#endif
#ifndef EQLB_PERSIST_OVERSUB
#define EQLB_PERSIST_OVERSUB 1 // persistent grid of k_se_patch_fused: this many times the resident workgroups of the device
#endif

// ---- tiled stress launch (eqlb_stress_tiled.hip) ----
#ifndef EQLB_STRESS_THREADS
#define EQLB_STRESS_THREADS 512 // threads of a workgroup of k_se_stress_tiled
#endif
#ifndef EQLB_STRESS_WAVES
#define EQLB_STRESS_WAVES 2 // waves per SIMD asked from the register allocator
#endif
#ifndef EQLB_STRESS_TILE_CELLS
#define EQLB_STRESS_TILE_CELLS 524 // largest stress tile (STRESS_TCMAX)
#endif

// ---- primal CG (eqlb_primal_solve.hip) ----
#ifndef EQLB_PRIMAL_CHECK_EVERY
// PRIMAL_CHECK_EVERY: iterations enqueued between two reads of the state by the host.  P_2 at 1M triangles to rtol 1e-8
// from zero (4 652 iterations, one run each in one call of tools/primal_solve_time.py --check-every): 1: 684.3 ms,
// 4: 623.4 ms, 16: 590.3 ms, 64: 588.3 ms.  16 and 64 are 0.4 % apart; the result does not depend on the value
#define EQLB_PRIMAL_CHECK_EVERY 64
#endif

// ---- the product with an assembled matrix (eqlb_primal_matrix.hip: k_csr_apply) ----
// CSR_GROUP: lanes that sum the rows of a bundle together (a power of two, 2 ... 64); CSR_GROUP_MIN: entries of the longest
// row of a bundle from which they do.  One eqlb_csr_apply at 1M triangles, ms, P_1 / P_2 Poisson, [P_1]^2 / [P_2]^2
// elasticity (7, 11.5, 14 and 23 entries per row; tools/matrix_time.py --product-only, medians of 5 blocks of 200 calls,
// one run each, spreads below 0.006):
//   one row per thread only   0.0209  0.2083  0.1043  1.3428
//   2, 16    0.0205  0.1762  0.0896  0.8175        2, 8     0.0253  0.1955  0.0929  0.8160
//   4, 16    0.0206  0.1641  0.0835  0.7453        4, 8     0.0259  0.2176  0.0916  0.7469
//   4, 12    0.0212  0.1717  0.0819  0.7441        4, 24    0.0206  0.1637  0.1035  0.7828
//   8, 16    0.0214  0.1737  0.0991  0.9080        8, 8     0.0350  0.2877  0.1270  0.9096
//   16, 24   0.0215  0.1906  0.1039  0.9501        16, 12   0.0216  0.2091  0.1523  1.3874
//   32, 24   0.0218  0.2249  0.1043  1.1504
// The result does not depend on the values: the sum of a row runs in the one order
#ifndef EQLB_CSR_GROUP
#define EQLB_CSR_GROUP 4
#endif
#ifndef EQLB_CSR_GROUP_MIN
#define EQLB_CSR_GROUP_MIN 16
#endif

// ---- exact solve on the coarsest level of a hierarchy (eqlb_coarse.hip) ----
#ifndef EQLB_COARSE_MAX_ROWS
#define EQLB_COARSE_MAX_ROWS 4096 // free rows of level 0 at the most: n^2 * 8 B per layout of the factor, two layouts (268 MB)
#endif
#ifndef EQLB_COARSE_BLOCK
#define EQLB_COARSE_BLOCK 32 // columns per step of the blocked LDL^T: the entries of a row of the panel in registers (2 ... 32)
#endif
#ifndef EQLB_COARSE_TILE
#define EQLB_COARSE_TILE 64 // rows and columns of a tile of the trailing updates (two operand tiles of 17 KB in LDS); threads of the per-row kernels (a multiple of 16, at most 64)
#endif

// ---- weak-symmetry kernels (eqlb_se_weaksym*.hip) ----
#ifndef EQLB_WS_LEAN_WAVES
#define EQLB_WS_LEAN_WAVES 2 // waves per SIMD asked for k_se_weaksym_lean
#endif
#ifndef EQLB_WS_PIVOT_RTOL
#define EQLB_WS_PIVOT_RTOL 1e-11 // relative size (against the largest entry of the Schur system) below which a pivot counts as zero
#endif
