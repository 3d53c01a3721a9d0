// The grid of the kernels that walk [channels][baselines] arrays in tiles of runs and chunks of
// rows (apply_gains, predict), the only place that knows it: what the launcher works out and
// what a thread makes of it.
//
// A workgroup of `threads` threads owns a tile of `tile_runs` runs of KSP_RUN baselines (a power
// of two, 1 .. max_tile_runs: the narrowest that holds a row) and a chunk of `chunk` rows. Its
// threads are dealt to a flat index over runs and rows: thread t owns run t % tile_runs of the
// tile and, of every batch of slots = threads / tile_runs rows, row t / tile_runs, so a narrow
// array still fills its wavefronts. The chunk is a multiple of `slots` chosen so that a launch
// has about `target_groups` workgroups where the array is large enough. Workgroups are numbered
// in a one-dimensional grid, tiles fastest.
#pragma once
#include "ksp_common.h"
#include "run16.h"

struct ksp_tile_geometry {
    int tile_shift;  // log2(tile_runs)
    int tiles;       // tiles per row
    int chunk;       // rows per workgroup
    long long groups;
};

// (groups stays below 3 * target_groups + tiles, and tiles is at most 2^27 / max_tile_runs)
static ksp_tile_geometry ksp_make_tile_geometry(int channels, int baselines, int threads,
                                                int max_tile_runs, int target_groups)
{
    ksp_tile_geometry g;
    const int runs_per_row = (int)(((long long)baselines + KSP_RUN - 1) / KSP_RUN);
    g.tile_shift = 0;
    while ((1 << g.tile_shift) < max_tile_runs && (1 << g.tile_shift) < runs_per_row) g.tile_shift++;
    const int tile_runs = 1 << g.tile_shift;
    g.tiles = (runs_per_row + tile_runs - 1) / tile_runs;
    const int slots = threads / tile_runs;  // rows a workgroup works on at once
    long long chunk = (long long)channels * g.tiles / target_groups / slots * slots;
    if (chunk > channels) chunk = channels;  // (wide rows: the tiles alone are groups enough)
    if (chunk < slots) chunk = slots;
    g.chunk = (int)chunk;
    g.groups = (channels + chunk - 1) / chunk * g.tiles;
    return g;
}

// Where a thread stands: its workgroup's tile and rows [row_begin, row_end), and its own run of
// the tile (columns col0 .. col0 + valid - 1) and row slot.
struct ksp_tile_place {
    int tile, run, slot, slots;
    long long row_begin, row_end;
    long long tile_col0, col0;  // (64-bit: lanes beyond the end of the last tile may pass 2^31)
    int valid;  // elements of the run inside the row: 0 for a lane beyond it
};

__device__ __forceinline__ ksp_tile_place ksp_tile_locate(int threads, int tiles, int tile_shift,
                                                          int chunk, int channels, int baselines)
{
    ksp_tile_place at;
    const int tid = threadIdx.x;
    at.tile = blockIdx.x % tiles;
    at.row_begin = (long long)(blockIdx.x / tiles) * chunk;
    at.row_end = min((long long)channels, at.row_begin + chunk);
    const int tile_runs = 1 << tile_shift;
    at.run = tid & (tile_runs - 1);
    at.slot = tid >> tile_shift;
    at.slots = threads >> tile_shift;
    at.tile_col0 = (long long)at.tile * (tile_runs * KSP_RUN);
    // (statements in this order and col0 in this form leave apply_gains' instructions as they
    // were before the two kernels shared this function)
    at.col0 = ((long long)at.tile * tile_runs + at.run) * KSP_RUN;
    at.valid = (int)min((long long)KSP_RUN, max(0ll, baselines - at.col0));
    return at;
}
