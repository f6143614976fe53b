// dph_geometry.h -- the constants the kernels and the host planning rules (dph_plan.h) share.  Plain C++: no HIP header, so that the
// rules compile -- and are tested -- with a host compiler alone.
#pragma once
#include <stdint.h>
#include "../../include/dph.h"             // DPH_DIM

// ---------------------------------------------------------------- geometry of the scan
// A scan workgroup is 4 waves, one per SIMD, one workgroup per CU.  Wave w owns QB groups of 32 query rows for the
// whole launch and keeps their HIGH int8 digit in registers (24 k-steps x 4 registers per group).  One launch ("pass")
// therefore serves 128*QB query rows: QB = 1 is the reference's eval batch (2B = 128 rows, index.py:196-197), QB = 2
// serves 256 rows with one read of the dump (BASELINE configs[3]/[4]: batches of 256 / 512 queries).
// Database rows stream HBM -> hand-owned AGPRs -> LDS in tiles of 32 rows = 24 KiB; every wave reads every tile.
#define DPH_KSTEPS 24               // 768 / 32 int8 per v_mfma_i32_32x32x32_i8
#define DPH_QGROUP 32               // query rows per MFMA column block
#define DPH_QROWS 128               // query rows per pass at QB = 1 (4 waves x 32)
#define DPH_MAX_QB 2
#define DPH_TILE_ROWS 32
#define DPH_TILE_BYTES (DPH_TILE_ROWS * DPH_DIM)     // 24576
#define DPH_SCAN_THREADS 256
#define DPH_QGROUP_FRAG_BYTES (DPH_KSTEPS * 64 * 16) // 24576: [kstep][lane][16 B] fragment image of one 32-row group
#define DPH_CENTER 40               // the code of x = 0 at the default codec ((0 - offset) * scale): centre of the synthetic dumps

// ---------------------------------------------------------------- bounds of the filter (round 5)
// Every bound is a Cauchy-Schwarz bound around the shard's PER-DIMENSION mean code mu (integers, dph_index_finalize):
//   <v, n> = <v, n - mu> + <v, mu> <= ||v||_2 * ||n - mu||_2 + <v, mu>,   <v, mu> exact per query row (dph_quantize_kernel).
// Shards whose rows are NOT alike -- rogue dimensions, heavy-tailed row norms -- additionally carry AUX ROWS (dph_scan.hip "the aux
// k-step"): `stride` bytes per stored row that a 25th k-step of the scan multiplies with the query row's aux digits, slot by slot.
#define DPH_AUX_SLOTS 32            // int8 slots of the aux k-step = bytes of a query row's aux digits
#define DPH_AUX_REP_MAX 24          // replica slots (further high digits of rogue dimensions)
struct dph_aux_layout {
    int stride;                     // bytes per stored row of the aux array: 0 = the shard has none, 4 = 4 norm slots, 16 = 4 norm + 12 replica slots, 32 = 8 + 24
    int n_norm;                     // slots [0, n_norm): codes of the row's centred norm, their sum = ceil(|| n - mu ||_2 / norm_unit)
    int n_rep;                      // slots [n_norm, n_norm + n_rep): the row's raw code in dimension rep_dim[s - n_norm]
    int q2max;                      // clamp of the low digit (64 unless the norm unit is large: the norm slots' query digit must fit int8)
    short rep_dim[DPH_AUX_REP_MAX]; // a dimension with R replica slots has 1 + R high digits: | q1 | <= 127 (1 + R)
};

// what the scan emits: one (row, query row) pair per database row whose high-digit score may beat the row's bound
// Pairs live in a POOL shared by all scan waves of a launch, handed out in chunks: a wave claims a chunk with one atomic
// when it first emits and again whenever its chunk is full, so a burst of hits in one wave (a workgroup streaming a whole
// inverted list of near neighbours, a run of near-duplicate rows) takes what it needs from the common store instead of
// overflowing a fixed per-wave region.  Rows lose pairs only when the whole pool is exhausted.
#define DPH_CHUNK_PAIRS 256         // pairs per chunk (2 KiB)
#define DPH_POOL_CHUNKS 32768       // chunks in the pool: 8 Mi pairs = 64 MiB
#define DPH_BUCKET_CAP 32768        // exact-integer-score keys per query row after the refine step (256 KiB)
#define DPH_POOL_MAX 8192           // keys the select kernel sorts in LDS
#define DPH_SELECT_C_MAX 2048       // candidates a retry pass re-scores in fp64 (first attempt: max(2k, k+32))
#define DPH_EXACT_ROWS_DEV 32       // rows per call the on-device fp64 fallback serves (rounds 1-4: 8; the rest: host loop / status 1)
#define DPH_EXACT_HEAD 1024         // bytes in front of the fallback's hit buffers: counters | redo flags | tightened thresholds
#define DPH_EXACT_HITS (1u << 20)   // boundary hits per such row the fallback's buffer holds (as before; 32 x 2^20 x 16 B = 512 MiB of 288 GB:
                                    // an all-zero query ties with every row of a shard of up to a million rows and must still be served)

// IVF unit scan (dph_scan_units_kernel): a pass serves up to DPH_PASS_MAX query rows.  Every probed inverted list is cut
// into CHUNKS of at most 128 probing query rows ("slots": the 4 x 32 MFMA columns of a scan workgroup) and into
// SEGMENTS of DPH_UNIT_TILES contiguous tiles; a UNIT = (chunk, segment) is what a scan workgroup takes from the
// work queue: it multiplies the tiles of the segment with the gathered high digits of the chunk's query rows only.
#define DPH_PASS_MAX 1024           // query rows per pass of the unit scan (and the size of every per-pass array)
#define DPH_UNIT_WORDS (DPH_PASS_MAX / 32)   // probe-mask words per list in that pass
#define DPH_UNIT_TILES 256          // tiles per segment (6 MiB of the dump; 1024 measured no better: the tail grows)
#define DPH_UNIT_SLOTS 128
#define DPH_UNIT_LAUNCHES 8         // work-queue counters per pass (one per scan launch: ladder levels + the full scan)

#define DPH_SAMPLE_KEEP 16          // scores per query row a rank shares for the union bound

#define DPH_NORM_BINS 8192          // histogram of squared centred row norms: bins of DPH_NORM_BIN_W (max 768*168^2 < 2^25)
#define DPH_NORM_BIN_W 4096u
#define DPH_OUTLIER_MAX 1024        // rows per shard that may be treated as outliers (always scored, never bounded)

// ---------------------------------------------------------------- the ADC scans of the PQ index (dph_pq.hip)
#define PQ_THREADS 1024
#define PQ_SEG 12288                  // codes per segment (M <= 96: 96 KiB of LUT + 48 KiB of keys); halved for larger M (LDS budget).  12288: a row-major unit of the released shape (64 lists, ~10 k codes) is ONE segment -- one k-th selection per unit instead of two (8192: r1-r4)
#define PQ_FINAL_CAP 4096             // candidates the final sort takes (k + boundary ties)
#define PQ_LM_CHUNK 4                 // segments of a list per (row, list) pair of the list-major scan (dph_pq.hip, pq_pairs_kernel)
#define PQ_GROUP 64                   // probed lists per group of the row-major scan (dph_pq.hip, pq_units_kernel)
