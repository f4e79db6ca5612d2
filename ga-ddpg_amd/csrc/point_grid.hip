// Plan, carve and build of the uniform point grid (point_grid.hpp; what a query relies on and the margins it keeps: with the two
// query kernels in ball_query.hip and interpolate.hip).  Six launches on the caller's stream, no host synchronisation, nothing sized by the data:
//   bounds   per-workgroup min / max over the points whose three coordinates are finite; clears the slice table
//   setup    one wavefront per cloud: the box, then a grid with <= PG_GMAX cells per axis and <= `cells` in all (the budget the
//            host derives from N alone), by one of two edge rules.
//            PG_EDGE_RADIUS: the finest grid of edge >= 1.002 r; coarsened by 1.25 x per try until it fits.
//            PG_EDGE_BUDGET: there is no radius: the cell edge is picked from the box of the finite points and the cell budget
//            (min(max(N / 4, 64), 65536): about four points per cell of a cloud that fills its box).  The first edge is the one
//            at which box volume / edge^3 (area / edge^2 and length / edge where one or two extents are zero) equals the budget,
//            at least extent / PG_GMAX; it is coarsened by 1.1 x per try until the cells, counted as the cell function counts
//            them, fit.  An axis of zero extent gets one cell, a box whose extent overflows ends in one cell (every point a
//            candidate of the first block: still exact).
//   count    STABLE ranks.  A cloud is cut into `slices` contiguous index ranges, one wavefront each, which walks its range in
//            index order 64 points at a time: the lanes of one cell are ranked by lane, and the slice's running count of that
//            cell -- a row of the table that belongs to this wavefront alone -- is advanced by the cell's lowest lane.  The
//            add is an integer atomic only so that the next 64 points read it coherently: no other wavefront touches the row
//            and the adds of one wavefront are issued one after another (each result is consumed before the next is issued),
//            so the value returned is the count over the slice's EARLIER points, whatever the rest of the chip does.
//   slices   per cell: exclusive prefix of the slices' counts in slice order (in place), total -> start[cell]
//   scan     one workgroup per cloud: exclusive prefix over the cells
//   scatter  sorted[start[cell] + prefix[slice][cell] + rank] = (x, y, z, index): a stable counting sort, indices ascending
//            inside every cell and the same array whatever the scheduling
#include "point_grid.hpp"
#include <algorithm>

__device__ __forceinline__ void pg_wave_minmax(float (&lo)[3], float (&hi)[3]) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64));
        }
}

__global__ __launch_bounds__(256) void pg_bounds_kernel(const float* __restrict__ xyz, int N, float* __restrict__ part,
                                                         int32_t* __restrict__ table, long long table_ints) {
    __shared__ float red[4][6];
    const int b = blockIdx.y, tid = threadIdx.x, parts = gridDim.x;
    const float* p = xyz + (size_t)b * N * 3;
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (int k = blockIdx.x * 256 + tid; k < N; k += parts * 256) {
        const float v[3] = {p[k * 3 + 0], p[k * 3 + 1], p[k * 3 + 2]};
        if (pg_finite(v[0]) && pg_finite(v[1]) && pg_finite(v[2])) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], v[a]); hi[a] = fmaxf(hi[a], v[a]); }
        }
    }
    pg_wave_minmax(lo, hi);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[tid >> 6][a] = lo[a]; red[tid >> 6][3 + a] = hi[a]; }
    }
    __syncthreads();
    if (tid < 6) {
        float v = red[0][tid];
        for (int w = 1; w < 4; ++w) v = tid < 3 ? fminf(v, red[w][tid]) : fmaxf(v, red[w][tid]);
        part[((size_t)b * parts + blockIdx.x) * 6 + tid] = v;
    }
    const long long me = (long long)blockIdx.y * parts + blockIdx.x, stride = (long long)gridDim.y * parts * 256;
    for (long long i = me * 256 + tid; i < table_ints; i += stride) table[i] = 0;
}

__device__ __forceinline__ int pg_axis(float ext, float inv) {   // cells of edge 1 / inv along an extent; NaN / huge -> over the cap
    const float f = ext * inv;
    return f < (float)(2 * PG_GMAX) ? (int)f + 1 : 2 * PG_GMAX + 1;
}

__global__ __launch_bounds__(64) void pg_setup_kernel(const float* __restrict__ part, int parts, int edge, float radius, int cells,
                                                      PointGrid* __restrict__ hdr, int32_t* __restrict__ stats) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    if (lane < parts) {
        const float* q = part + ((size_t)b * parts + lane) * 6;
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = q[a]; hi[a] = q[3 + a]; }
    }
    pg_wave_minmax(lo, hi);
    if (lane != 0) return;
    if (edge == PG_EDGE_BUDGET && stats) { stats[b * 2] = 0; stats[b * 2 + 1] = 0; }
    if (!(hi[0] >= lo[0])) {                                      // a cloud without a finite point: one cell at the origin
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = hi[a] = 0.f;
    }
    const float e[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};                 // >= 0; +inf where the box overflows
    float h = radius * 1.002f, grow = 1.25f, emax = 0.f;           // PG_EDGE_RADIUS: 1.25^512 covers the whole float range
    int tries = 512, dims = 0;
    if (edge == PG_EDGE_BUDGET) {
        // the edge at which the box, over the axes it extends along, is cut into `cells` cells (roots first: no overflow)
        h = 1.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (e[a] > 0.f) { ++dims; emax = fmaxf(emax, e[a]); }
        }
        if (dims == 3) {
            h = cbrtf(e[0]) * cbrtf(e[1]) * cbrtf(e[2]) / cbrtf((float)cells);
        } else if (dims == 2) {
#pragma unroll
            for (int a = 0; a < 3; ++a) h *= e[a] > 0.f ? sqrtf(e[a]) : 1.f;
            h /= sqrtf((float)cells);
        } else if (dims == 1) {
            h = emax / (float)cells;
        }
        h = fmaxf(h, emax * (1.0f / (float)PG_GMAX));
        if (!(h > 1.0e-30f)) h = 1.0e-30f;                        // (1 / h stays finite)
        grow = 1.1f; tries = 256;                                 // (the first edge is within 1024 x of one that fits)
    }
    float inv = 0.f;
    int nx = 1, ny = 1, nz = 1;
    bool fits = false;
    for (int it = 0; it < tries && !fits; ++it) {
        inv = 1.0f / h;
        nx = pg_axis(e[0], inv); ny = pg_axis(e[1], inv); nz = pg_axis(e[2], inv);
        fits = nx <= PG_GMAX && ny <= PG_GMAX && nz <= PG_GMAX && (long long)nx * ny * nz <= (long long)cells;
        h *= grow;
    }
    if (!fits) { nx = ny = nz = 1; inv = 0.f; }                  // (an infinite extent: every point in the one cell)
    PointGrid g;
    g.lox = lo[0]; g.loy = lo[1]; g.loz = lo[2];
    g.ivx = g.ivy = g.ivz = inv;
    g.nx = nx; g.ny = ny; g.nz = nz; g.ncells = nx * ny * nz;
#pragma unroll
    for (int a = 0; a < 6; ++a) g.reserved_[a] = 0;
    hdr[b] = g;
}

__global__ __launch_bounds__(64) void pg_count_kernel(const float* __restrict__ xyz, int N, int slices, int slice, int cells,
                                                       const PointGrid* __restrict__ hdr, int32_t* __restrict__ cellof,
                                                       int32_t* __restrict__ rank, int32_t* __restrict__ table) {
    const int b = blockIdx.x / slices, q = blockIdx.x - b * slices, lane = threadIdx.x;
    const PointGrid g = hdr[b];
    const float* p = xyz + (size_t)b * N * 3;
    int32_t* row = table + ((size_t)b * slices + q) * cells;
    int32_t* co = cellof + (size_t)b * N;
    int32_t* rk = rank + (size_t)b * N;
    const int k0 = q * slice, k1 = min(N, k0 + slice);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = k0; base < k1; base += 64) {
        const int k = base + lane;
        const bool live = k < k1;
        int cell = -1;
        if (live)
            cell = (pg_cell1(p[k * 3 + 2], g.loz, g.ivz, g.nz) * g.ny + pg_cell1(p[k * 3 + 1], g.loy, g.ivy, g.ny)) * g.nx +
                   pg_cell1(p[k * 3 + 0], g.lox, g.ivx, g.nx);
        // the lanes of one cell: rank by lane, the lowest lane leads
        int before = 0, total = 0, leader = lane;
        unsigned long long todo = __ballot(live);
        while (todo) {                                            // wave-uniform
            const int l0 = __ffsll((long long)todo) - 1;
            const int c0 = __shfl(cell, l0, 64);
            const unsigned long long m = __ballot(live && cell == c0);
            if (live && cell == c0) { before = __popcll(m & below); total = __popcll(m); leader = l0; }
            todo &= ~m;
        }
        int seen = 0;                                             // points of this cell earlier in the slice
        if (live && leader == lane) seen = __hip_atomic_fetch_add(row + cell, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        seen = __shfl(seen, leader, 64);                          // (consumes the result: the next group's adds follow it)
        if (live) { co[k] = cell; rk[k] = seen + before; }
    }
}

__global__ __launch_bounds__(256) void pg_slices_kernel(int slices, int cells, const PointGrid* __restrict__ hdr,
                                                         int32_t* __restrict__ table, int32_t* __restrict__ start) {
    const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= hdr[b].ncells) return;
    int32_t* t = table + (size_t)b * slices * cells + c;
    int run = 0;
    for (int q = 0; q < slices; ++q) {
        const int v = t[(size_t)q * cells];
        t[(size_t)q * cells] = run;
        run += v;
    }
    start[(size_t)b * (cells + 1) + c] = run;
}

__global__ __launch_bounds__(1024) void pg_scan_kernel(int N, int cells, const PointGrid* __restrict__ hdr,
                                                        int32_t* __restrict__ start) {
    __shared__ int sums[1024];
    const int b = blockIdx.x, tid = threadIdx.x, n = hdr[b].ncells;
    int32_t* s = start + (size_t)b * (cells + 1);
    const int per = (n + 1023) / 1024, c0 = min(n, tid * per), c1 = min(n, c0 + per);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += s[c];
    sums[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? sums[tid - o] : 0;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    int run = sums[tid] - sum;
    for (int c = c0; c < c1; ++c) {
        const int v = s[c];
        s[c] = run;
        run += v;
    }
    if (tid == 0) s[n] = N;
}

__global__ __launch_bounds__(256) void pg_scatter_kernel(const float* __restrict__ xyz, int N, int slices, int slice, int cells,
                                                          const int32_t* __restrict__ cellof, const int32_t* __restrict__ rank,
                                                          const int32_t* __restrict__ table, const int32_t* __restrict__ start,
                                                          float4* __restrict__ sorted) {
    const int b = blockIdx.y;
    const float* p = xyz + (size_t)b * N * 3;
    const int32_t* t = table + (size_t)b * slices * cells;
    const int32_t* s = start + (size_t)b * (cells + 1);
    for (int k = blockIdx.x * 256 + threadIdx.x; k < N; k += gridDim.x * 256) {
        const int cell = cellof[(size_t)b * N + k];
        const int pos = s[cell] + t[(size_t)(k / slice) * cells + cell] + rank[(size_t)b * N + k];
        if ((unsigned)pos < (unsigned)N)                           // (always: the three terms count disjoint sets of earlier points)
            sorted[(size_t)b * N + pos] = make_float4(p[k * 3 + 0], p[k * 3 + 1], p[k * 3 + 2], __int_as_float(k));
    }
}

static long long pg_up(long long v) { return (v + 255) & ~255ll; }
int point_grid_plan(const char* who, int B, int N, PointGridPlan* pl) {
    GAD_REQUIRE(B >= 0 && N >= 1, GAD_ERR_SHAPE, "%s: no grid over B=%d clouds of N=%d points", who, B, N);
    GAD_REQUIRE((long long)N * 3 < (1ll << 31) && (long long)B * N < (1ll << 31), GAD_ERR_SHAPE,
                "%s: B * N = %d * %d points (or 3 * N) overflows 32-bit indexing", who, B, N);
    pl->parts = (int)std::min<long long>(PG_MAXPARTS, gad_cdiv(N, 4096));
    pl->slices = (int)std::min<long long>(PG_MAXSLICES, gad_cdiv(N, 2048));
    pl->slice = gad_cdiv(gad_cdiv(N, pl->slices), 64) * 64;
    pl->cells = std::max(64, std::min(PG_MAXCELLS, N / 4));
    long long o = pg_up((long long)B * pl->parts * 6 * 4);                              // bounding-box partials at offset 0
    pl->o_hdr = o;    o += pg_up((long long)B * (long long)sizeof(PointGrid));
    pl->o_cellof = o; o += pg_up((long long)B * N * 4);
    pl->o_rank = o;   o += pg_up((long long)B * N * 4);
    pl->o_table = o;  o += pg_up((long long)B * pl->slices * pl->cells * 4);
    pl->o_start = o;  o += pg_up((long long)B * (pl->cells + 1) * 4);
    pl->o_sorted = o; o += pg_up((long long)B * N * 16 + 16);                           // (+16: the float4 array is aligned inside)
    pl->total = o;
    return GAD_OK;
}

int point_grid_carve(const char* who, void* workspace, const PointGridPlan& pl, PointGridView* v) {
    GAD_REQUIRE(workspace, GAD_ERR_NULL, "%s: null pointer (workspace)", who);
    GAD_REQUIRE((reinterpret_cast<size_t>(workspace) & 7) == 0, GAD_ERR_SHAPE, "%s: the workspace must be 8-byte aligned", who);
    char* w = static_cast<char*>(workspace);
    v->part = reinterpret_cast<float*>(w);
    v->hdr = reinterpret_cast<PointGrid*>(w + pl.o_hdr);
    v->cellof = reinterpret_cast<int32_t*>(w + pl.o_cellof);
    v->rank = reinterpret_cast<int32_t*>(w + pl.o_rank);
    v->table = reinterpret_cast<int32_t*>(w + pl.o_table);
    v->start = reinterpret_cast<int32_t*>(w + pl.o_start);
    v->sorted = reinterpret_cast<float4*>((reinterpret_cast<size_t>(w + pl.o_sorted) + 15) & ~(size_t)15);
    return GAD_OK;
}

void point_grid_build(const float* cloud, int B, int N, const PointGridPlan& pl, const PointGridView& v, PointGridEdge edge,
                      float radius, int32_t* stats, hipStream_t st) {
    const int pt_grid = (int)std::min<long long>(1024, gad_cdiv(N, 256));
    hipLaunchKernelGGL(pg_bounds_kernel, dim3(pl.parts, B), dim3(256), 0, st, cloud, N, v.part, v.table,
                       (long long)B * pl.slices * pl.cells);
    hipLaunchKernelGGL(pg_setup_kernel, dim3(B), dim3(64), 0, st, v.part, pl.parts, (int)edge, radius, pl.cells, v.hdr, stats);
    hipLaunchKernelGGL(pg_count_kernel, dim3(B * pl.slices), dim3(64), 0, st, cloud, N, pl.slices, pl.slice, pl.cells, v.hdr, v.cellof,
                       v.rank, v.table);
    hipLaunchKernelGGL(pg_slices_kernel, dim3(gad_cdiv(pl.cells, 256), B), dim3(256), 0, st, pl.slices, pl.cells, v.hdr, v.table, v.start);
    hipLaunchKernelGGL(pg_scan_kernel, dim3(B), dim3(1024), 0, st, N, pl.cells, v.hdr, v.start);
    hipLaunchKernelGGL(pg_scatter_kernel, dim3(pt_grid, B), dim3(256), 0, st, cloud, N, pl.slices, pl.slice, pl.cells, v.cellof, v.rank,
                       v.table, v.start, v.sorted);
}
