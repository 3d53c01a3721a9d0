// Tile transposition fused with the caller's own loads and stores (HIP, gfx950).
//
// Counterpart of the reference's transpose_base.mako. A work-group of BLOCK x BLOCK
// work-items moves one tile of BLOCK * VTY rows by BLOCK * VTX columns of the source
// through LDS and writes it as BLOCK * VTX rows by BLOCK * VTY columns of the
// destination. The caller supplies what happens to each element on the way in and on
// the way out as lambdas `(r, c, lr, lc)`: (r, c) are coordinates in global memory (of
// the source in load, of the destination in store), (lr, lc) index the LDS tile, and
// neither pair is ever to be swapped by the caller. Bounds checks belong to the lambda.
//
//     LOCAL_DECL ksp::transpose_tile<float, BLOCK, VTX, VTY> tile;
//     ksp::transpose_coords<BLOCK, VTX, VTY> coords;
//     coords.init_simple();
//     coords.load([&](int r, int c, int lr, int lc) {
//         if (r < in_rows && c < in_cols) tile.arr[lr][lc] = in[r * in_stride + c];
//     });
//     BARRIER();
//     coords.store([&](int r, int c, int lr, int lc) {
//         if (r < in_cols && c < in_rows) out[r * out_stride + c] = tile.arr[lr][lc];
//     });
//
// Launch geometry (the reference's): local size (BLOCK, BLOCK), one work-group per tile,
// ceil(in_cols / (BLOCK * VTX)) groups in x by ceil(in_rows / (BLOCK * VTY)) groups in
// y. Group (x, y) takes tile row (x + y) % groups_y, so that groups running side by
// side spread over the memory channels; every tile is still visited exactly once.
#pragma once
#include "port.h"

namespace ksp
{

namespace detail
{
// Row pitch of the LDS tile, in elements. In the store phase lane (lx, ly) reads
// arr[lx + ..][ly + ..]: consecutive lanes walk down a column. The LDS serves 32 lanes at
// a time (ds_read_b128: 16) from banks of 4 bytes, 32 of them for ds_read_b32 and 64 for
// the 8- and 16-byte reads, i.e. 32 (16) distinct slots of max(4, sizeof(T)) bytes. For
// BLOCK < 32 such a group of lanes spans G = 32 / BLOCK values of ly, which land on
// neighbouring slots, so the pitch must move each next lx by G slots and never wrap onto
// a used one: a pitch of G times an odd number of slots. Sub-dword elements are padded
// to whole dwords first; lanes that then share a dword read the same address, which
// the LDS broadcasts. (The row-order writes of the load phase can collide two ways
// under such a pitch; an LDS store is bound by moving its registers, at twice the
// array's time, so that does not cost.)
constexpr int transpose_pitch(int elem_size, int block, int vtx)
{
    const int slot = elem_size > 4 ? elem_size : 4;
    const int per_slot = slot / elem_size;
    const bool pow2 = (block & (block - 1)) == 0;
    const int g = pow2 && block < 32 ? 32 / block : 1;
    int n = (block * vtx + per_slot * g - 1) / (per_slot * g);  // slots, in units of g
    if (n % 2 == 0) n++;
    return n * g * per_slot;
}
}  // namespace detail

/// The data of one tile; declare it LOCAL_DECL. Several tiles of plain element types
/// serve a kernel better than one tile of a struct.
template <class T, int BLOCK, int VTX, int VTY> struct transpose_tile
{
    static constexpr int rows = BLOCK * VTY;
    static constexpr int cols = BLOCK * VTX;
    static constexpr int pitch = detail::transpose_pitch(sizeof(T), BLOCK, VTX);
    T arr[rows][pitch];
};

/// Addressing of one work-item; lives in registers.
template <int BLOCK, int VTX, int VTY> struct transpose_coords
{
    int lx;       ///< local x within the block (fastest varying)
    int ly;       ///< local y within the block
    int in_row0;  ///< first source row of the tile
    int in_col0;  ///< first source column of the tile

    /// Explicit local and block coordinates; blocks_y is the number of tile rows.
    DEVICE_FN void init(int local_x, int local_y, int block_x, int block_y, int blocks_y)
    {
        lx = local_x;
        ly = local_y;
        in_row0 = (block_x + block_y) % blocks_y * (BLOCK * VTY);
        in_col0 = block_x * (BLOCK * VTX);
    }

    /// Coordinates taken from the launch.
    DEVICE_FN void init_simple()
    {
        init(get_local_id(0), get_local_id(1), get_group_id(0), get_group_id(1),
             get_num_groups(1));
    }

    /// body(r, c, lr, lc) once per sub-tile: (r, c) in the source, (lr, lc) in the tile.
    template <class Body> DEVICE_FN void load(Body &&body) const
    {
#pragma unroll
        for (int y = 0; y < VTY; y++)
#pragma unroll
            for (int x = 0; x < VTX; x++)
                body(in_row0 + y * BLOCK + ly, in_col0 + x * BLOCK + lx, y * BLOCK + ly,
                     x * BLOCK + lx);
    }

    /// body(r, c, lr, lc) once per sub-tile: (r, c) in the destination, (lr, lc) in the
    /// tile. Consecutive lanes take consecutive destination columns, i.e. tile rows.
    template <class Body> DEVICE_FN void store(Body &&body) const
    {
#pragma unroll
        for (int y = 0; y < VTX; y++)
#pragma unroll
            for (int x = 0; x < VTY; x++)
                body(in_col0 + y * BLOCK + ly, in_row0 + x * BLOCK + lx, x * BLOCK + lx,
                     y * BLOCK + ly);
    }
};

}  // namespace ksp
