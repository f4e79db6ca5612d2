// The uniform point grid: every cloud of a batch sorted once into cells in the caller's workspace, for operators that search around
// a point of a cloud no workgroup can hold.  What a query kernel and its entry point need; point_grid.hip: the build, its derivation.
#pragma once
#include "common.hpp"
#define PG_GMAX 1024                               // cells per axis
#define PG_MAXCELLS 65536                          // cells per cloud
#define PG_MAXSLICES 64                            // index ranges per cloud (count pass)
#define PG_MAXPARTS 64                             // bounding-box partials per cloud

// per cloud: cell (x, y, z) = pg_cell1 of each coordinate, its points are sorted[start[(z * ny + y) * nx + x] .. start[.. + 1])
struct PointGrid { float lox, loy, loz, ivx, ivy, ivz; int32_t nx, ny, nz, ncells; int32_t reserved_[6]; };
static_assert(sizeof(PointGrid) == 64, "the workspace layout counts 64 bytes per cloud");

__device__ __forceinline__ bool pg_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
// monotone in p, in [0, n) for every p (NaN -> 0)
__device__ __forceinline__ int pg_cell1(float p, float lo, float inv, int n) {
    const float f = (p - lo) * inv;
    return f >= (float)(n - 1) ? n - 1 : (f > 0.f ? (int)f : 0);
}
__device__ __forceinline__ void pg_wave_sync() {                  // LDS written by some lanes of a wavefront, read by others
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// shapes, launch geometry and workspace layout (byte offsets, each a multiple of 256) of one call
struct PointGridPlan { int parts, slices, slice, cells; long long o_hdr, o_cellof, o_rank, o_table, o_start, o_sorted, total; };
// a carved workspace: box partials, headers, cell and rank of every point, slice counts, cell starts, points (x, y, z, index) by cell
struct PointGridView { float* part; PointGrid* hdr; int32_t *cellof, *rank, *table, *start; float4* sorted; };
// how the setup launch picks the first cell edge: 1.002 x `radius`, or from the box of the finite points and the cell budget
enum PointGridEdge { PG_EDGE_RADIUS = 0, PG_EDGE_BUDGET = 1 };

// the index-range checks of (B, N) and the layout; `who` names the caller, which itself refuses B > 65535 (a cloud is a grid row)
int point_grid_plan(const char* who, int B, int N, PointGridPlan* pl);
// refuses a NULL or misaligned workspace, else fills *v
int point_grid_carve(const char* who, void* workspace, const PointGridPlan& pl, PointGridView* v);
// enqueues bounds, setup, count, slices, scan, scatter over cloud (B, N, 3); PG_EDGE_BUDGET also zeroes stats[2 * B] if given
void point_grid_build(const float* cloud, int B, int N, const PointGridPlan& pl, const PointGridView& v, PointGridEdge edge,
                      float radius, int32_t* stats, hipStream_t st);
