// flag_count: how many samples of a uint8 flag array [rows][stride] have a bit of a mask
// set, per row and per column, for up to 8 masks, in one pass over the flags (no reference
// counterpart: the reference leaves counting to its callers, who do it on a host copy).
//
//   row_counts[m][r] = #{ c : flags[r][c] & masks[m] != 0 }
//   col_counts[m][c] = #{ r : flags[r][c] & masks[m] != 0 }
//
// Tile. A 256-thread workgroup walks FC_TILE_COLS = 4096 columns x `tile_rows` rows: lane
// t of the workgroup owns the 16 bytes at columns 16 t .. 16 t + 15 of every row of the tile
// (one global_load_dwordx4 per row; a wavefront reads 1 KiB of a row, the workgroup 4 KiB),
// FC_UNROLL rows in flight per lane. The launcher picks tile_rows from the shape so that
// the grid has about four workgroups per CU (fc_tile_rows()).
//
// Per byte. The four 32-bit words of a row piece are tested as packed bytes: with
// t = w & (mask * 0x01010101) the bytes of ((t | ((t & 0x7f7f7f7f) + 0x7f7f7f7f)) >> 7)
// & 0x01010101 are 1 where the byte of t is non-zero (0x7f + 0x7f = 0xfe: nothing carries
// into the next byte; bit 7 itself comes in through the OR). When every mask has one bit
// the word is (w & mask4) >> bit.
//
// Column counts. That word is added to a packed-byte accumulator per (mask, word): a byte
// of it counts one column over the rows of the tile, at most FC_MAX_TILE_ROWS = 128 < 255,
// so it cannot overflow. At the end of the tile the bytes are widened to 32 bits through
// LDS, which also turns "lane t holds 16 adjacent columns" into "lane t holds column
// k * 256 + t", and added to col_counts with atomicAdd: a wavefront adds to 64 adjacent
// counters (256 contiguous bytes) per instruction.
//
// Row counts. A lane's count for a row is the population count of its four words; two
// rows share a register (16-bit fields: a wavefront's total is at most 1024), one DPP
// reduction per pair of rows sums over the wavefront, and the pairs of an unrolled step go to
// LDS in one add by as many lanes, where the four wavefronts of the workgroup meet (at most
// 4096 per row: the 16-bit fields hold). At the end thread r adds row r of the tile to
// row_counts, again on adjacent counters.
//
// Integer sums do not depend on their order, so the result is exact and the same on every
// run. Sums wrap modulo 2^32 (only reachable with accumulate, or more than 2^32 - 1 rows
// or columns, which the int arguments exclude).
//
// The 16 bytes of a lane are a run of run16.h: unaligned input and the lanes at the right-hand
// edge load byte by byte, and padding is never read, let alone counted.
#include "launch.h"
#include "run16.h"

#define FC_THREADS 256
#define FC_TILE_COLS (FC_THREADS * 16)
#define FC_MAX_TILE_ROWS 128
#define FC_UNROLL 8
#define FC_MAX_MASKS 8
#define FC_TARGET_WORKGROUPS 1024  // four per CU of an MI355X

struct fc_masks {
    unsigned mask4[FC_MAX_MASKS];  // the mask in each byte of a word
    unsigned shift[FC_MAX_MASKS];  // bit number of a one-bit mask
};

template <bool SINGLE_BIT>
__device__ __forceinline__ unsigned fc_nonzero_bytes(unsigned w, unsigned mask4, unsigned shift)
{
    const unsigned t = w & mask4;
    if (SINGLE_BIT) return t >> shift;
    return ((t | ((t & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u;
}

// UNROLL (even) rows are in flight per lane. FULL: every lane of the wavefront has all 16 bytes
// of its run, on 16-byte boundaries.
template <int NM, bool SINGLE_BIT, bool FULL, int UNROLL>
__device__ __forceinline__ void fc_walk(const uint8_t *base, long long stride, int nrows, int valid,
                                        const fc_masks &masks, unsigned (&acc)[NM][4],
                                        unsigned (*lds_rows)[FC_MAX_TILE_ROWS / 2], int lane)
{
    for (int r = 0; r < nrows; r += UNROLL) {
        ksp_run_bytes v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            v[u] = ksp_run_bytes{0, 0, 0, 0};
            if (r + u < nrows)
                v[u] = ksp_run_load_bytes(base + (long long)(r + u) * stride,
                                          FULL ? KSP_RUN : valid, FULL);
        }
#pragma unroll
        for (int m = 0; m < NM; m++) {
            unsigned mine = 0;  // lane j: the wavefront's counts of rows r + 2 j, r + 2 j + 1
#pragma unroll
            for (int u = 0; u < UNROLL; u += 2) {
                unsigned pair = 0;
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    unsigned count = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const unsigned nz = fc_nonzero_bytes<SINGLE_BIT>(
                            v[u + h][k], masks.mask4[m], masks.shift[m]);
                        acc[m][k] += nz;
                        count += __builtin_popcount(nz);
                    }
                    pair |= count << (16 * h);
                }
                const unsigned total = (unsigned)ksp_wave_sum_dpp((int)pair);
                mine = lane == u / 2 ? total : mine;
            }
            // (rows beyond nrows were loaded as zeros and r + UNROLL <= FC_MAX_TILE_ROWS)
            if (lane < UNROLL / 2) atomicAdd(&lds_rows[m][(r >> 1) + lane], mine);
            // One mask at a time. Left alone, the compiler sums the words of the UNROLL rows
            // as a tree after the last mask, which keeps 4 * UNROLL registers per mask alive.
#pragma unroll
            for (int k = 0; k < 4; k++) asm volatile("" : "+v"(acc[m][k]));
        }
    }
}

template <int NM, bool SINGLE_BIT>
__global__ __launch_bounds__(FC_THREADS) void flag_count_kernel(
    const uint8_t *__restrict__ flags, unsigned *__restrict__ row_counts,
    unsigned *__restrict__ col_counts, int rows, int cols, long long stride,
    long long row_counts_stride, long long col_counts_stride, int tile_rows, unsigned col_tiles,
    int aligned, fc_masks masks)
{
    __shared__ unsigned lds_rows[NM][FC_MAX_TILE_ROWS / 2];
    __shared__ unsigned lds_cols[FC_TILE_COLS];
    const int tid = threadIdx.x;
    const int lane = tid % KSP_WAVE;
    const unsigned col_tile = blockIdx.x % col_tiles;
    const unsigned row_tile = blockIdx.x / col_tiles;
    const int row0 = (int)row_tile * tile_rows;  // < rows
    const int nrows = min(tile_rows, rows - row0);
    const long long tile_col0 = (long long)col_tile * FC_TILE_COLS;  // < cols
    const long long col0 = tile_col0 + tid * 16;
    const int valid = (int)max(0ll, min(16ll, (long long)cols - col0));

    for (int i = tid; i < NM * (FC_MAX_TILE_ROWS / 2); i += FC_THREADS) (&lds_rows[0][0])[i] = 0;
    __syncthreads();

    unsigned acc[NM][4];
#pragma unroll
    for (int m = 0; m < NM; m++)
#pragma unroll
        for (int k = 0; k < 4; k++) acc[m][k] = 0;

    // (a lane with nothing to load never dereferences its pointer)
    const uint8_t *base = flags + (long long)row0 * stride + col0;
    // both conditions are the same for every lane of a wavefront: fc_walk's reductions see
    // all 64 lanes
    if (aligned && !ksp_any(valid != 16))
        fc_walk<NM, SINGLE_BIT, true, FC_UNROLL>(base, stride, nrows, valid, masks, acc, lds_rows, lane);
    else if (ksp_any(valid > 0))
        fc_walk<NM, SINGLE_BIT, false, 2>(base, stride, nrows, valid, masks, acc, lds_rows, lane);
    __syncthreads();

    if (tid < nrows) {
#pragma unroll
        for (int m = 0; m < NM; m++) {
            const unsigned count = (lds_rows[m][tid >> 1] >> (16 * (tid & 1))) & 0xffffu;
            atomicAdd(row_counts + m * row_counts_stride + row0 + tid, count);
        }
    }
#pragma unroll
    for (int m = 0; m < NM; m++) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned a = acc[m][k];
            *reinterpret_cast<uint4 *>(&lds_cols[tid * 16 + 4 * k]) =
                make_uint4(a & 0xffu, (a >> 8) & 0xffu, (a >> 16) & 0xffu, a >> 24);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int c = k * FC_THREADS + tid;
            if (tile_col0 + c < cols)
                atomicAdd(col_counts + m * col_counts_stride + tile_col0 + c, lds_cols[c]);
        }
        __syncthreads();
    }
}

// Rows per tile: as many as leave the grid FC_TARGET_WORKGROUPS workgroups, in whole
// unrolled steps, between 32 (64 with several masks: every tile costs 16 KiB of atomic
// adds per mask, 1/8 byte per byte of flags at 32 rows) and FC_MAX_TILE_ROWS.
static int fc_tile_rows(int rows, long long col_tiles, int n_masks)
{
    const long long row_tiles = (FC_TARGET_WORKGROUPS + col_tiles - 1) / col_tiles;
    long long t = (rows + row_tiles - 1) / row_tiles;
    t = (t + FC_UNROLL - 1) / FC_UNROLL * FC_UNROLL;
    const long long lo = n_masks > 1 ? 64 : 32;
    return (int)(t < lo ? lo : t > FC_MAX_TILE_ROWS ? FC_MAX_TILE_ROWS : t);
}

extern "C" int ksp_flag_count(int device, void *stream, const uint8_t *flags, uint32_t *row_counts,
                              uint32_t *col_counts, int rows, int cols, int stride,
                              int row_counts_stride, int col_counts_stride, const uint8_t *masks,
                              int n_masks, int accumulate)
{
    KSP_REQUIRE(flags != nullptr, "flags is NULL");
    KSP_REQUIRE(row_counts != nullptr, "row_counts is NULL");
    KSP_REQUIRE(col_counts != nullptr, "col_counts is NULL");
    KSP_REQUIRE(masks != nullptr, "masks is NULL");
    KSP_REQUIRE(rows >= 1, "rows must be at least 1");
    KSP_REQUIRE(cols >= 1, "cols must be at least 1");
    KSP_REQUIRE(stride >= cols, "stride is smaller than cols");
    KSP_REQUIRE(row_counts_stride >= rows, "row_counts_stride is smaller than rows");
    KSP_REQUIRE(col_counts_stride >= cols, "col_counts_stride is smaller than cols");
    KSP_REQUIRE(n_masks >= 1 && n_masks <= FC_MAX_MASKS, "n_masks must be between 1 and 8");
    fc_masks packed = {};
    bool single_bit = true;
    for (int m = 0; m < n_masks; m++) {
        KSP_REQUIRE(masks[m] != 0, "a mask is zero");
        packed.mask4[m] = masks[m] * 0x01010101u;
        packed.shift[m] = (unsigned)__builtin_ctz(masks[m]);
        single_bit = single_bit && (masks[m] & (masks[m] - 1)) == 0;
    }
    const long long col_tiles = ((long long)cols + FC_TILE_COLS - 1) / FC_TILE_COLS;
    const int tile_rows = fc_tile_rows(rows, col_tiles, n_masks);
    const long long tiles = col_tiles * (((long long)rows + tile_rows - 1) / tile_rows);
    KSP_REQUIRE(tiles <= 0x7fffffffll, "array too large for one launch");
    const int aligned = ksp_rows_aligned(flags, stride, 1);

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    if (!accumulate) {
        // only the counters themselves: the padding of the outputs is not ours to write
        KSP_CHECK(hipMemset2DAsync(row_counts, (size_t)row_counts_stride * 4, 0, (size_t)rows * 4,
                                   (size_t)n_masks, s));
        KSP_CHECK(hipMemset2DAsync(col_counts, (size_t)col_counts_stride * 4, 0, (size_t)cols * 4,
                                   (size_t)n_masks, s));
    }
    const dim3 grid((unsigned)tiles);
    // (n_masks is 1 .. FC_MAX_MASKS here)
    ksp_dispatch_exact<1, 2, 3, 4, 5, 6, 7, 8>(n_masks, [&](auto NM) {
        ksp_dispatch_bool(single_bit, [&](auto SINGLE_BIT) {
            hipLaunchKernelGGL((flag_count_kernel<decltype(NM)::value, SINGLE_BIT()>), grid,
                               dim3(FC_THREADS), 0, s, flags, row_counts, col_counts, rows, cols,
                               (long long)stride, (long long)row_counts_stride,
                               (long long)col_counts_stride, tile_rows, (unsigned)col_tiles,
                               aligned, packed);
        });
    });
    KSP_LAUNCH_CHECK();
    return 0;
}
