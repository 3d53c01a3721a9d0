// sir: the scale-invariant rank operator (Offringa, van de Gronde & Roerdink 2012) on a uint8
// flag array [rows][stride], in place, along either axis (no reference counterpart: the
// semantics are those of rfi/host.py ScaleInvariantRankHost, matched bit for bit).
//
// A line is f[0..n). With psi_i = eta_q if f[i] & mask, else eta_q - 4096, and M(j) the sum
// of psi_i over i < j (int32: |M| <= n * 4096 <= 2^30), sample x is in the result iff
//
//   R(x) = max over b in (x, n] of M(b)  >=  L(x) = min over a in [0, x] of M(a)
//
// and then gets flags[x] |= flag_value. L runs forward and R backward, so every sample
// needs something from either end of its line. A stretch of the line is summarised by
// (t, lo, hi): the sum of its psi and the smallest and largest of its prefix sums, the empty
// prefix and the whole one included. Summaries compose, so a line is cut into pieces; what a
// piece needs from the rest of the line is M at its start, L at its start and R at its end.
//
// Leaf. 16 samples of one line in registers (SIR_LEAF): a forward walk keeps L for each of
// them, a backward walk carries R and decides. A leaf is loaded whole before any byte of it
// is stored, and everything upstream of a store has read the stored bytes for the last time,
// so flag_value may overlap mask.
//
// Samples beyond the end of a line are loaded as zero, i.e. unflagged. That is exact: such a
// position p > n has M(p) <= M(n) (psi of an unflagged sample is not positive), so it never
// raises a maximum, and no minimum over [0, x], x < n, reaches it.
//
// axis 0 (lines down the columns). A workgroup of 16 wavefronts owns SIR0_TILE_COLS = 128
// columns: a lane owns two adjacent columns (one 2-byte load per row, a wavefront reads one
// 128-byte line of a row), which gives 256 workgroups of 16 wavefronts for 32768 columns:
// one workgroup per CU of an MI355X, four wavefronts per SIMD. Four or 16 bytes per lane would
// leave half or seven eighths of the CUs without a workgroup. The rows are cut into panels
// of 16 parts, one part per wavefront, a part being `leaves` (1..16, from the row count)
// leaves of 16 rows. A wavefront summarises its part leaf by leaf, keeping in registers the
// running minimum in front of every leaf (2 x 16 values), the 16 summaries meet in LDS, every
// lane combines them for its two columns, and the wavefront walks its leaves backward:
// two reads and one write of the flags for up to 4096 rows. Longer lines take one more read:
// a forward pass over all panels leaves L at the start of every panel in LDS (at most 64
// panels), then the panels are done last to first, carrying M and R.
//
// axis 1 (lines along the rows). A workgroup of 256 threads per line, thread t owning the 16
// bytes at 16 t of a segment of 4096 samples (one global_load_dwordx4). The 256 leaf
// summaries are combined with three wavefront scans (sum, minimum, and maximum from the far
// end) and an LDS step over the four wavefronts; the loaded bytes stay in registers, so a
// line of up to 4096 samples is read once and written once. Longer lines take segments the way
// axis 0 takes panels: a forward pass, then last to first.
//
// Unaligned input (odd pointer or stride for axis 0, not multiples of 16 for axis 1, whose
// leaves are runs of run16.h) and the lanes at the ragged end of a row load and store byte by
// byte, and only bytes inside the row: padding is neither read nor written.
#include <limits.h>

#include <utility>

#include "launch.h"
#include "run16.h"

#define SIR_MAX_LINE 262144
#define SIR_LEAF 16
#define SIR_NONE INT_MIN  // "no position": the maximum over an empty set

#define SIR0_WAVES 16
#define SIR0_THREADS (SIR0_WAVES * KSP_WAVE)
#define SIR0_TILE_COLS (2 * KSP_WAVE)
#define SIR0_MAX_LEAVES 16  // per wavefront and panel: 1, 2, 4, 8 or 16 (a template argument)
#define SIR0_MAX_PANELS (SIR_MAX_LINE / (SIR0_WAVES * SIR_LEAF * SIR0_MAX_LEAVES))

#define SIR1_THREADS 256
#define SIR1_WAVES (SIR1_THREADS / KSP_WAVE)
#define SIR1_SEGMENT (SIR1_THREADS * SIR_LEAF)
#define SIR1_MAX_SEGMENTS (SIR_MAX_LINE / SIR1_SEGMENT)

struct sir_params {
    int base;        // psi of an unflagged sample, eta_q - 4096; a flagged one has 4096 more
    unsigned mask;
    unsigned value;  // flag_value
};

__device__ __forceinline__ int sir_psi(unsigned fbits, int i, int base)
{
    return base + (int)(((fbits >> i) & 1u) << 12);
}

// Extends the summary (t, lo, hi) by the samples of a leaf; bit i of fbits: sample i is flagged.
__device__ __forceinline__ void sir_leaf_sum(unsigned fbits, int base, int &t, int &lo, int &hi)
{
#pragma unroll
    for (int i = 0; i < SIR_LEAF; i++) {
        t += sir_psi(fbits, i, base);
        lo = min(lo, t);
        hi = max(hi, t);
    }
}

// Which samples of a leaf are in the result, as bits. m: M at its first sample; l: the minimum
// of M over [0, first sample) (anything not below it will do when m is not above it); r: the
// maximum of M over [end of the leaf, n], left as the maximum over [first sample, n].
__device__ __forceinline__ unsigned sir_leaf_decide(unsigned fbits, int base, int m, int l, int &r)
{
    int lmin[SIR_LEAF];
#pragma unroll
    for (int i = 0; i < SIR_LEAF; i++) {
        l = min(l, m);
        lmin[i] = l;
        m += sir_psi(fbits, i, base);
    }
    // (The way back subtracts what the way forward added, from the same bits: seen through,
    // the compiler keeps the 16 psi and the 16 values of m in registers instead.)
    asm volatile("" : "+v"(m), "+v"(fbits));
    unsigned out = 0;
#pragma unroll
    for (int i = SIR_LEAF - 1; i >= 0; i--) {
        out |= (unsigned)(r >= lmin[i]) << i;
        m -= sir_psi(fbits, i, base);
        r = max(r, m);
    }
    return out;
}

// What one of `count` consecutive pieces needs from the others, from their summaries
// sum(k) = (t, lo, hi), k = 0 .. count - 1, relative to the start of the first piece:
// mine.t = M at the start of piece `which`, mine.lo = the minimum of M up to there, mine.hi =
// the maximum of M over the pieces behind it (SIR_NONE for the last); all = the summary of
// the lot.
struct sir_sum {
    int t, lo, hi;
};
template <typename F>
__device__ __forceinline__ void sir_combine(int count, int which, F &&sum, sir_sum &mine,
                                            sir_sum &all)
{
    int m = 0, lo = 0, hi = 0;
    mine.t = 0, mine.lo = 0, mine.hi = SIR_NONE;
    // (unrolled all the way, the 16 x 3 x 2 LDS reads of axis 0 are all in flight at once
    // and take 96 registers)
#pragma unroll 4
    for (int k = 0; k < count; k++) {
        const sir_sum s = sum(k);
        if (k == which) mine.t = m, mine.lo = lo;
        if (k > which) mine.hi = max(mine.hi, m + s.hi);
        lo = min(lo, m + s.lo);
        hi = max(hi, m + s.hi);
        m += s.t;
    }
    all.t = m, all.lo = lo, all.hi = hi;
}

// r_end of a piece: the maximum behind the group of pieces, or one inside it
__device__ __forceinline__ int sir_r_end(int r_group, int m_group, int hi_behind)
{
    return hi_behind == SIR_NONE ? r_group : max(r_group, m_group + hi_behind);
}

// ---------------------------------------------------------------------------- axis 0
// A pointer that is the same for every lane of the wavefront, as a scalar the compiler no
// longer sees through: `p[lane's 32-bit offset]` is then the scalar-base form of global_load
// and global_store. Left to itself the compiler folds the lane's offset into a 64-bit address
// per row, two registers for every access in flight.
// (Global address space by name: a pointer made from an integer is a flat one otherwise.)
typedef __attribute__((address_space(1))) uint8_t sir_global_u8;
typedef __attribute__((address_space(1))) unsigned short sir_global_u16;
__device__ __forceinline__ sir_global_u8 *sir_scalar(const uint8_t *p)
{
    const unsigned long long a = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return (sir_global_u8 *)(((unsigned long long)hi << 32) | lo);
}

// A lane's two columns: the tile's first column (the same for the whole wavefront: row
// offsets are added to it in scalar arithmetic, and global_load takes a scalar base) and
// the lane's own byte offsets. Loads do not branch on the lane: a column beyond `cols` is read
// at the tile's first column instead, which exists, and masked to zero by `live`. PAIR: both columns in one 2-byte access (the launcher takes
// it when pointer, stride and `cols` are even, so a lane has both columns or neither).
template <bool PAIR>
struct sir0_column {
    uint8_t *tile;
    unsigned offset[2];
    unsigned live;  // 0xff per column inside `cols`
    int valid;      // how many of the two are

    __device__ __forceinline__ sir0_column(uint8_t *flags, int cols, int lane)
    {
        const long long tile_col0 = (long long)blockIdx.x * SIR0_TILE_COLS;  // < cols
        tile = flags + tile_col0;
        valid = (int)max(0ll, min(2ll, cols - tile_col0 - 2 * lane));
        offset[0] = valid > 0 ? 2u * lane : 0u;
        offset[1] = valid > 1 ? 2u * lane + 1u : offset[0];
        live = valid > 1 ? 0xffffu : valid > 0 ? 0xffu : 0u;
    }
    // The same columns with offsets the compiler knows nothing of, for the accesses of one
    // leaf: it then widens them to 64 bits where they are used (and folds that into the
    // access: a scalar base and a 32-bit offset), not once for the whole kernel (then every
    // access would add two 64-bit registers).
    __device__ __forceinline__ sir0_column fresh() const
    {
        sir0_column c = *this;
        asm volatile("" : "+v"(c.offset[0]), "+v"(c.offset[1]));
        return c;
    }
    // the two bytes in the low half of a word
    __device__ __forceinline__ unsigned load(long long row_offset) const
    {
        const sir_global_u8 *row = sir_scalar(tile + row_offset);
        if (PAIR) return *(const sir_global_u16 *)(row + offset[0]) & live;
        return (row[offset[0]] | ((unsigned)row[offset[1]] << 8)) & live;
    }
};

// Rows row0 .. row0 + 15 of a lane's two columns (rows at and beyond `rows` as zero), and
// which of them are flagged, per column.
template <bool PAIR>
__device__ __forceinline__ void sir0_load_leaf(const sir0_column<PAIR> &col, long long stride,
                                               int row0, int rows, unsigned mask,
                                               unsigned (&raw)[SIR_LEAF], unsigned (&fbits)[2])
{
    const sir0_column<PAIR> here = col.fresh();
    // Rows beyond the line: the last row once more, masked to zero. All of it in scalar
    // arithmetic that stays cheap: the row offset advances by the stride or by nothing, and
    // the mask is a word for an AND, from a shift (written as a comparison it becomes a lane
    // mask in a pair of scalar registers, 16 pairs to a leaf, and those run out).
    const int n_rows = rows - row0;
    long long row_offset = (long long)min(row0, rows - 1) * stride;
#pragma unroll
    for (int i = 0; i < SIR_LEAF; i++) {
        raw[i] = here.load(row_offset) & (unsigned)((i - n_rows) >> 31);
        row_offset += i + 1 < n_rows ? stride : 0;
    }
    fbits[0] = fbits[1] = 0;
#pragma unroll
    for (int i = 0; i < SIR_LEAF; i++) {
        fbits[0] |= (unsigned)((raw[i] & mask) != 0) << i;
        fbits[1] |= (unsigned)((raw[i] & (mask << 8)) != 0) << i;
    }
    // the walks take their samples from these bits: seen through, the compiler keeps the 32
    // comparisons (and their psi) alive instead, per leaf, and runs out of registers
    asm volatile("" : "+v"(fbits[0]), "+v"(fbits[1]));
}

// f(std::integral_constant<int, J>()) for J = 0 .. N - 1: a loop whose index is a constant from
// the start, not only once it has been unrolled. An array indexed by it is taken apart into
// separate registers; indexed by the variable of an unrolled loop it becomes one value as wide
// as the array, which is allocated, spilled and reloaded as a whole.
template <int... J, typename F>
__device__ __forceinline__ void sir_each(std::integer_sequence<int, J...>, F &&f)
{
    (f(std::integral_constant<int, J>()), ...);
}
template <int N, typename F>
__device__ __forceinline__ void sir_each(F &&f)
{
    sir_each(std::make_integer_sequence<int, N>(), f);
}

// The summary of a wavefront's part (LEAVES leaves of 16 rows from row0) for the lane's two
// columns, and the minimum of the prefix sums in front of each leaf, relative to the start of
// the part. Straight-line code (LEAVES is a template argument, rows beyond the line are
// samples like any other), so that lo_before stays 2 x LEAVES separate registers: assigned
// under branches it becomes one wide value that is spilled and reloaded as a whole.
template <bool PAIR, int LEAVES>
__device__ __forceinline__ void sir0_summarise(const sir0_column<PAIR> &col, long long stride,
                                               int row0, int rows, const sir_params &par,
                                               sir_sum (&sum)[2], int (&lo_before)[LEAVES][2])
{
#pragma unroll
    for (int c = 0; c < 2; c++) sum[c].t = 0, sum[c].lo = 0, sum[c].hi = 0;
    sir_each<LEAVES>([&](auto J) {
        constexpr int j = J();
        lo_before[j][0] = sum[0].lo;
        lo_before[j][1] = sum[1].lo;
        unsigned raw[SIR_LEAF], fbits[2];
        sir0_load_leaf<PAIR>(col, stride, row0 + j * SIR_LEAF, rows, par.mask, raw, fbits);
#pragma unroll
        for (int c = 0; c < 2; c++) sir_leaf_sum(fbits[c], par.base, sum[c].t, sum[c].lo, sum[c].hi);
    });
}

template <bool PAIR, int LEAVES>
__global__ __launch_bounds__(SIR0_THREADS) void sir_columns_kernel(
    uint8_t *__restrict__ flags, int rows, int cols, long long stride, int panels, sir_params par)
{
    __shared__ int lds_sum[SIR0_WAVES][3][SIR0_TILE_COLS];
    __shared__ int lds_panel_lo[SIR0_MAX_PANELS][SIR0_TILE_COLS];
    const int lane = threadIdx.x % KSP_WAVE;
    // (as a scalar: everything about rows, their addresses included, is scalar arithmetic)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / KSP_WAVE);
    const sir0_column<PAIR> col(flags, cols, lane);
    constexpr int part_rows = LEAVES * SIR_LEAF;
    constexpr int panel_rows = SIR0_WAVES * part_rows;

    sir_sum sum[2];
    const auto publish = [&]() {
#pragma unroll
        for (int c = 0; c < 2; c++) {
            lds_sum[wave][0][2 * lane + c] = sum[c].t;
            lds_sum[wave][1][2 * lane + c] = sum[c].lo;
            lds_sum[wave][2][2 * lane + c] = sum[c].hi;
        }
        __syncthreads();
    };
    const auto combine = [&](int c, sir_sum &mine, sir_sum &all) {
        sir_combine(SIR0_WAVES, wave, [&](int k) {
            return sir_sum{lds_sum[k][0][2 * lane + c], lds_sum[k][1][2 * lane + c],
                           lds_sum[k][2][2 * lane + c]};
        }, mine, all);
    };

    // M at the end of the panel in hand and the maximum of M from there on, per column
    int m_end[2] = {0, 0}, r_end[2] = {0, 0};
    if (panels > 1) {
        int lo_run[2] = {0, 0};
        for (int p = 0; p < panels; p++) {
            int lo_before[LEAVES][2];  // (not used by this pass)
            sir0_summarise<PAIR, LEAVES>(col, stride, p * panel_rows + wave * part_rows, rows, par,
                                         sum, lo_before);
            publish();
#pragma unroll
            for (int c = 0; c < 2; c++) {
                sir_sum mine, all;
                combine(c, mine, all);
                if (wave == 0) lds_panel_lo[p][2 * lane + c] = lo_run[c];
                lo_run[c] = min(lo_run[c], m_end[c] + all.lo);
                m_end[c] += all.t;
            }
            __syncthreads();
        }
        r_end[0] = m_end[0];
        r_end[1] = m_end[1];
    }

    for (int p = panels - 1; p >= 0; p--) {
        const int row0 = p * panel_rows + wave * part_rows;
        int lo_before[LEAVES][2];
        sir0_summarise<PAIR, LEAVES>(col, stride, row0, rows, par, sum, lo_before);
        publish();
        int m[2], l[2], r[2], m_part[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            sir_sum mine, all;
            combine(c, mine, all);
            if (panels == 1) m_end[c] = r_end[c] = all.t;  // one panel: it starts at M = 0
            const int m_panel = m_end[c] - all.t;
            const int l_panel = panels > 1 ? lds_panel_lo[p][2 * lane + c] : 0;
            m_part[c] = m_panel + mine.t;
            l[c] = min(l_panel, m_panel + mine.lo);
            r[c] = sir_r_end(r_end[c], m_panel, mine.hi);
            m[c] = m_part[c] + sum[c].t;  // at the end of the part: the leaves go backward
            r_end[c] = max(r_end[c], m_panel + all.hi);
            m_end[c] = m_panel;
        }
        __syncthreads();  // (lds_sum is free for the next panel)
        sir_each<LEAVES>([&](auto J) {
            constexpr int j = LEAVES - 1 - J();
            const int leaf_row0 = row0 + j * SIR_LEAF;
            unsigned raw[SIR_LEAF], fbits[2], out[2];
            sir0_load_leaf<PAIR>(col, stride, leaf_row0, rows, par.mask, raw, fbits);
#pragma unroll
            for (int c = 0; c < 2; c++) {
                m[c] -= SIR_LEAF * par.base + (__builtin_popcount(fbits[c]) << 12);
                out[c] = sir_leaf_decide(fbits[c], par.base, m[c],
                                         min(l[c], m_part[c] + lo_before[j][c]), r[c]);
                // The decisions as 16 bits, here: left to itself the compiler moves every
                // comparison down to the store of its row, and the 16 minima and 16 maxima
                // of both columns stay in registers until then.
                asm volatile("" : "+v"(out[c]));
            }
#pragma unroll
            for (int i = 0; i < SIR_LEAF; i++)
                raw[i] |= (((out[0] >> i) & 1u) | (((out[1] >> i) & 1u) << 8)) * par.value;
            // Stores: the only branches on a lane's columns (one or two per leaf) and on rows
            // (n_rows is not positive for a leaf beyond the line).
            const int n_rows = rows - leaf_row0;
            const sir0_column<PAIR> here = col.fresh();
            if (PAIR) {
                if (col.valid > 0) {
                    long long row_offset = (long long)leaf_row0 * stride;
#pragma unroll
                    for (int i = 0; i < SIR_LEAF; i++) {
                        if (i < n_rows)
                            *(sir_global_u16 *)(sir_scalar(col.tile + row_offset) + here.offset[0]) =
                                (unsigned short)raw[i];
                        row_offset += stride;
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    if (col.valid > c) {
                        long long row_offset = (long long)leaf_row0 * stride;
#pragma unroll
                        for (int i = 0; i < SIR_LEAF; i++) {
                            if (i < n_rows)
                                sir_scalar(col.tile + row_offset)[here.offset[c]] =
                                    (uint8_t)(raw[i] >> (8 * c));
                            row_offset += stride;
                        }
                    }
                }
            }
        });
    }
}

// ---------------------------------------------------------------------------- axis 1
__device__ __forceinline__ unsigned sir1_fbits(const unsigned (&w)[4], unsigned mask)
{
    unsigned fbits = 0;
#pragma unroll
    for (int i = 0; i < 16; i++)
        fbits |= (unsigned)((w[i / 4] & (mask << (8 * (i % 4)))) != 0) << i;
    return fbits;
}

// From every thread's leaf summary `own` to what its leaf needs from the segment (`mine`, as
// sir_combine gives it for pieces) and the summary of the segment. Every thread of the
// workgroup calls it; `lds` is free again when it returns.
__device__ __forceinline__ void sir1_scan(const sir_sum &own, int (*lds)[3], sir_sum &mine,
                                          sir_sum &all)
{
    const int lane = threadIdx.x % KSP_WAVE;
    const int wave = threadIdx.x / KSP_WAVE;
    const int incl = ksp_wave_scan_dpp(own.t);
    const int m = incl - own.t;  // M at the start of the leaf, relative to the wavefront's first
    const int lo_incl = ksp_wave_scan_min_dpp(m + own.lo);
    // the maximum over this lane and those behind it: a prefix scan on the mirrored wavefront
    const int hi_incl =
        __shfl(ksp_wave_scan_max_dpp(__shfl(m + own.hi, KSP_WAVE - 1 - lane, KSP_WAVE)),
               KSP_WAVE - 1 - lane, KSP_WAVE);
    const int lo_up = __shfl_up(lo_incl, 1, KSP_WAVE);
    const int hi_down = __shfl_down(hi_incl, 1, KSP_WAVE);
    const int lo_before = lane == 0 ? m : lo_up;  // (a leaf's lo covers its end, the next one's start)
    const int hi_behind = lane == KSP_WAVE - 1 ? SIR_NONE : hi_down;
    const int t_wave = __builtin_amdgcn_readlane(incl, KSP_WAVE - 1);
    const int lo_wave = __builtin_amdgcn_readlane(lo_incl, KSP_WAVE - 1);
    if (lane == 0) {
        lds[wave][0] = t_wave;
        lds[wave][1] = lo_wave;
        lds[wave][2] = hi_incl;
    }
    __syncthreads();
    sir_sum of_wave;
    sir_combine(SIR1_WAVES, wave, [&](int k) { return sir_sum{lds[k][0], lds[k][1], lds[k][2]}; },
                of_wave, all);
    __syncthreads();
    mine.t = of_wave.t + m;
    mine.lo = min(of_wave.lo, of_wave.t + lo_before);
    mine.hi = hi_behind == SIR_NONE ? of_wave.hi : max(of_wave.hi, of_wave.t + hi_behind);
}

template <bool ALIGNED>
__global__ __launch_bounds__(SIR1_THREADS) void sir_rows_kernel(uint8_t *__restrict__ flags,
                                                                int cols, long long stride,
                                                                int segments, sir_params par)
{
    __shared__ int lds_sum[SIR1_WAVES][3];
    __shared__ int lds_segment_lo[SIR1_MAX_SEGMENTS];
    uint8_t *line = flags + (long long)blockIdx.x * stride;
    const int tid = threadIdx.x;

    const auto load = [&](int segment, unsigned (&w)[4], int &valid) {
        const int col0 = segment * SIR1_SEGMENT + tid * SIR_LEAF;  // < 2^18 + 2^12
        valid = max(0, min(SIR_LEAF, cols - col0));
        const ksp_run_bytes v = ksp_run_load_bytes(line + col0, valid, ALIGNED);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        return col0;
    };

    int m_end = 0, r_end = 0;  // M at the end of the segment in hand, the maximum from there on
    if (segments > 1) {
        int lo_run = 0;
        for (int p = 0; p < segments; p++) {
            unsigned w[4];
            int valid;
            load(p, w, valid);
            sir_sum own = {0, 0, 0}, mine, all;
            sir_leaf_sum(sir1_fbits(w, par.mask), par.base, own.t, own.lo, own.hi);
            sir1_scan(own, lds_sum, mine, all);
            if (tid == 0) lds_segment_lo[p] = lo_run;
            lo_run = min(lo_run, m_end + all.lo);
            m_end += all.t;
        }
        r_end = m_end;
        __syncthreads();
    }

    for (int p = segments - 1; p >= 0; p--) {
        unsigned w[4];
        int valid;
        const int col0 = load(p, w, valid);
        const unsigned fbits = sir1_fbits(w, par.mask);
        sir_sum own = {0, 0, 0}, mine, all;
        sir_leaf_sum(fbits, par.base, own.t, own.lo, own.hi);
        sir1_scan(own, lds_sum, mine, all);
        if (segments == 1) m_end = r_end = all.t;  // one segment: it starts at M = 0
        const int m_segment = m_end - all.t;
        const int l_segment = segments > 1 ? lds_segment_lo[p] : 0;
        int r = sir_r_end(r_end, m_segment, mine.hi);
        const unsigned out = sir_leaf_decide(fbits, par.base, m_segment + mine.t,
                                             min(l_segment, m_segment + mine.lo), r);
#pragma unroll
        for (int i = 0; i < SIR_LEAF; i++) w[i / 4] |= (((out >> i) & 1u) * par.value) << (8 * (i % 4));
        ksp_run_store_bytes(line + col0, valid, ALIGNED, ksp_run_bytes{w[0], w[1], w[2], w[3]});
        r_end = max(r_end, m_segment + all.hi);
        m_end = m_segment;
    }
}

extern "C" int ksp_sir(int device, void *stream, uint8_t *flags, int rows, int cols, int stride,
                       int axis, int eta_q, int mask, int flag_value)
{
    KSP_REQUIRE(flags != nullptr, "flags is NULL");
    KSP_REQUIRE(axis == 0 || axis == 1, "axis must be 0 or 1");
    KSP_REQUIRE(rows >= 1, "rows must be at least 1");
    KSP_REQUIRE(cols >= 1, "cols must be at least 1");
    KSP_REQUIRE(stride >= cols, "stride is smaller than cols");
    KSP_REQUIRE((axis == 0 ? rows : cols) <= SIR_MAX_LINE, "line longer than 262144 samples");
    KSP_REQUIRE(eta_q >= 0 && eta_q <= 4096, "eta_q must be between 0 and 4096");
    KSP_REQUIRE(mask >= 1 && mask <= 255, "mask must be between 1 and 255");
    KSP_REQUIRE(flag_value >= 1 && flag_value <= 255, "flag_value must be between 1 and 255");
    const sir_params par = {eta_q - 4096, (unsigned)mask, (unsigned)flag_value};

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    if (axis == 0) {
        // leaves per wavefront and panel: as few (of 1, 2, 4, 8, 16) as put the line into one
        // panel
        const int per_leaf = SIR0_WAVES * SIR_LEAF;  // rows of a panel per leaf of its parts
        const int want = min(SIR0_MAX_LEAVES, (rows + per_leaf - 1) / per_leaf);
        const dim3 grid((unsigned)(((long long)cols + SIR0_TILE_COLS - 1) / SIR0_TILE_COLS));
        const bool pair = ksp_rows_aligned(flags, stride, 1, 2) && cols % 2 == 0;
        ksp_dispatch_ceil<1, 2, 4, 8, SIR0_MAX_LEAVES>(want, [&](auto L) {
            constexpr int panel_rows = per_leaf * L();
            const int panels = (rows + panel_rows - 1) / panel_rows;  // <= SIR0_MAX_PANELS
            ksp_dispatch_bool(pair, [&](auto PAIR) {
                hipLaunchKernelGGL((sir_columns_kernel<PAIR(), decltype(L)::value>), grid,
                                   dim3(SIR0_THREADS), 0, s, flags, rows, cols, (long long)stride,
                                   panels, par);
            });
        });
    } else {
        const int segments = (cols + SIR1_SEGMENT - 1) / SIR1_SEGMENT;  // <= SIR1_MAX_SEGMENTS
        const dim3 grid((unsigned)rows);
        ksp_dispatch_bool(ksp_rows_aligned(flags, stride, 1), [&](auto ALIGNED) {
            hipLaunchKernelGGL(sir_rows_kernel<ALIGNED()>, grid, dim3(SIR1_THREADS), 0, s, flags,
                               cols, (long long)stride, segments, par);
        });
    }
    KSP_LAUNCH_CHECK();
    return 0;
}
