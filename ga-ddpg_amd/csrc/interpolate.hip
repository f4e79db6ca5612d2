// Feature propagation: gad_three_nn (exhaustive, tiled through LDS), gad_three_nn_grid (point grid in global memory),
// gad_three_interpolate and its gradients.  Replaces upstream interpolate_gpu.cu.
#include "common.hpp"
#include "point_grid.hpp"
#include <algorithm>

// ------------------------------------------------------------------------------------------------
// feature propagation: three nearest neighbours + inverse-distance interpolation (+grad)
// (upstream interpolate_gpu.cu: three_nn_kernel, three_interpolate_kernel, three_interpolate_grad_kernel)
// ------------------------------------------------------------------------------------------------
// One lane per query point.  The known cloud passes through LDS in tiles of TNN_TILE points stored as (x, y, z, -): every lane
// reads the same address (one broadcast ds_read_b128 per point).  A lane walks the known points in ascending index order and keeps
// the three smallest (d, index) pairs in registers with upstream's strict-< insertion, so ties go to the lower index and a NaN
// distance is never taken.  Slots start at (+inf, 0): what upstream's 1e40 double becomes when stored as a float.
#define TNN_TILE 1024
__global__ __launch_bounds__(256) void three_nn_kernel(const float* __restrict__ unknown, const float* __restrict__ known, int n,
                                                       int m, int tiles, float* __restrict__ dist2, int32_t* __restrict__ idx) {
    __shared__ float4 kS[TNN_TILE];
    const int b = blockIdx.x / tiles, t = threadIdx.x;
    const int i = (blockIdx.x - b * tiles) * 256 + t;
    const float* u = unknown + ((size_t)b * n + min(i, n - 1)) * 3;          // lanes past n compute on the last point, store nothing
    const float ux = u[0], uy = u[1], uz = u[2];
    const float* kb = known + (size_t)b * m * 3;
    const float inf = __builtin_huge_valf();
    float d0 = inf, d1 = inf, d2 = inf;
    int i0 = 0, i1 = 0, i2 = 0;
    for (int k0 = 0; k0 < m; k0 += TNN_TILE) {
        const int nt = min(TNN_TILE, m - k0);
        __syncthreads();                                 // the previous tile consumed
        for (int j = t; j < nt; j += 256) {
            const float* p = kb + (size_t)(k0 + j) * 3;
            kS[j] = make_float4(p[0], p[1], p[2], 0.f);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < nt; ++j) {
            const float4 p = kS[j];
            const float d = gad_sqdist(ux, uy, uz, p.x, p.y, p.z);
            if (d < d2) {
                const int k = k0 + j;
                if (d < d0) {
                    d2 = d1; i2 = i1; d1 = d0; i1 = i0; d0 = d; i0 = k;
                } else if (d < d1) {
                    d2 = d1; i2 = i1; d1 = d; i1 = k;
                } else {
                    d2 = d; i2 = k;
                }
            }
        }
    }
    if (i < n) {
        const size_t o = ((size_t)b * n + i) * 3;
        dist2[o] = d0; dist2[o + 1] = d1; dist2[o + 2] = d2;
        idx[o] = i0; idx[o + 1] = i1; idx[o + 2] = i2;
    }
}

extern "C" int gad_three_nn(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx, void* stream) {
    GAD_REQUIRE(unknown && known && dist2 && idx, GAD_ERR_NULL, "three_nn: null pointer");
    GAD_REQUIRE(B >= 0 && n >= 0 && m >= 0, GAD_ERR_SHAPE, "three_nn: negative size (B %d, n %d, m %d)", B, n, m);
    if ((long long)B * n == 0) return GAD_OK;
    GAD_REQUIRE(m >= 1, GAD_ERR_SHAPE, "three_nn: no known point (m = %d) for %d queries", m, n);
    const int tiles = gad_cdiv(n, 256);
    GAD_REQUIRE((long long)B * tiles < (1ll << 31), GAD_ERR_SHAPE, "three_nn: B * n too large");
    hipLaunchKernelGGL(three_nn_kernel, dim3(B * tiles), dim3(256), 0, (hipStream_t)stream, unknown, known, n, m, tiles, dist2, idx);
    GAD_CHECK_LAUNCH("three_nn");
    return GAD_OK;
}

// ------------------------------------------------------------------------------------------------
// three_nn of large clouds: the uniform grid of point_grid.hpp over the KNOWN points, searched ring by ring
// ------------------------------------------------------------------------------------------------
// three_nn_kernel evaluates all n * m distances.  Here each cloud's known points are sorted once into a uniform grid -- the six
// launches of point_grid_build, the cell edge picked from the box and the cell budget (there is no radius: point_grid.hip) --
// and a wavefront per query tests the 3 x 3 x 3 cells around the query's (clamped) cell, then the shells of cells around that
// block, until no unexamined point can enter the answer.  Seven launches on the caller's stream, no host synchronisation,
// nothing sized by the data.
//   query    a candidate is the 64-bit key (bits of d) << 32 | index: d = gad_sqdist >= +0 in the pinned order, so unsigned
//            order of the keys IS the total order (d, index), and every key of a d that is +inf or NaN is >= the empty slot's
//            key (+inf, 0) and fails the strict < of the insertion.  Each lane keeps the three smallest keys of the candidates
//            it saw, a wavefront merge gives the three smallest of all: the result of three_nn_kernel's sequential strict-<
//            insertion, in whatever order the candidates are visited (every cell is visited once: no key twice).
// Stop test.  After ring r the examined block is cells [i - r, i + r] of every axis, cut to the grid.  An unexamined point lies
// beyond a face of the block that is not a border of the grid (border cells hold everything beyond them: the cell function is
// monotone and clamped).  With t = (p - lo) * inv in exact arithmetic, a point beyond the low (high) face of an axis has
// t < i - r (t >= i + r + 1) and the query t >= f (<= f), f its computed cell coordinate: along that axis they are `face`
// = f - (i - r) (or i + r + 1 - f) cells apart.  Along each OTHER axis any point of the cloud has 0 <= t < n, n the cells of the
// axis, so it is at least `out` = max(0, -f, f - n) cells from the query: what a query outside the box gains (without it such
// a query, clamped to a border cell, would never see a bound as large as its distance to the box and would always fall back).
// A point beyond a face is therefore at least sqrt(face^2 + out'^2 + out''^2) cells away, and the bound is the least of that
// over the non-border faces.  Rounding: f is clamped to [-2048, 3072] first -- towards the box: every term only shrinks -- so
// the computed (p - lo) * inv (two roundings, 1.2e-7 relative) is off by < 3.7e-4 cells for the query and, at <= PG_GMAX
// cells per axis, < 1.3e-4 for a point (the same holds for the extent, whose computed cell count is < n), and a difference
// of f and an integer by < 1.9e-4 more (one rounding at <= 3072): 6.9e-4 cells in all, TNN_CELL_SLACK = 1e-3 is taken off every
// term.  With c2 the resulting sum of squares the point is at least L = sqrt(c2) / inv away, and its d, five roundings of
// non-negative terms, is >= L * L * (1 - 3e-7).  The bound used is L * L * 0.99999 (1e-5 covers the 3e-7 and the roundings of
// forming c2, the root and L * L), ignored below 1e-30, where squares leave the normal range; an L * L that overflows stands
// for a bound no float reaches.  The search stops when the third-best d is STRICTLY below the bound -- a point at equal d
// and lower index would have to win -- or when the block covers the grid (fewer than three finite points, m < 3).  Every slack
// makes the bound smaller: one ring too many, never one too few.
// A query with a non-finite coordinate has no finite d: (+inf, 0) x 3 without a search.  A query unresolved after TNN_RINGS
// rings (far outside the box, in a large void) is redone by the wavefront walking all m known points: exact, only slower.
#define TNN_RINGS 3                                // (2 * 3 + 1)^2 = 49 (y, z) rows of a shell: one lane each
#define TNN_CELL_SLACK 1.0e-3f
#define TNN_INF_KEY 0x7f80000000000000ull          // (+inf, index 0): an unfilled slot
#define TNN_WAVES_TARGET 65536                     // wavefronts of the query launch where B * n allows (each takes a run of queries)

typedef unsigned long long tnn_key;

// (k0, k1, k2) <- the three smallest of {k0 <= k1 <= k2, k}: compare-exchanges, no branch (and no slot picked by an index)
__device__ __forceinline__ void tnn_insert(tnn_key k, tnn_key& k0, tnn_key& k1, tnn_key& k2) {
    tnn_key t = k0 < k ? k : k0;
    k0 = k0 < k ? k0 : k;
    const tnn_key u = k1 < t ? t : k1;
    k1 = k1 < t ? k1 : t;
    k2 = k2 < u ? k2 : u;
}
__device__ __forceinline__ tnn_key tnn_make_key(float d, int k) { return ((tnn_key)__float_as_uint(d) << 32) | (unsigned)k; }

__device__ __forceinline__ tnn_key tnn_wave_min(tnn_key v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        const tnn_key w = ((tnn_key)hi << 32) | lo;
        v = w < v ? w : v;
    }
    // (every lane holds the minimum: say so to the compiler, the branches on it are then scalar)
    return ((tnn_key)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}
// the three smallest keys over the lanes' lists (which stay as they are); every filled key is unique: one lane pops per round
__device__ __forceinline__ void tnn_wave_best3(tnn_key a0, tnn_key a1, tnn_key a2, tnn_key& g0, tnn_key& g1, tnn_key& g2) {
    g0 = tnn_wave_min(a0);
    if (a0 == g0) { a0 = a1; a1 = a2; a2 = TNN_INF_KEY; }
    g1 = tnn_wave_min(a0);
    if (a0 == g1) { a0 = a1; a1 = a2; }
    g2 = tnn_wave_min(a0);
}

// every lane brings one run [rs, rs + rl) of the sorted cloud (rl = 0: none); the wavefront walks the runs' points 64 at a time
__device__ __forceinline__ void tnn_scan_runs(const float4* __restrict__ sp, int m, int rs, int rl, int lane, float ux, float uy,
                                              float uz, tnn_key& k0, tnn_key& k1, tnn_key& k2) {
    int incl = rl;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    const int T = min(__builtin_amdgcn_readfirstlane(__shfl(incl, 63, 64)), m);   // (the runs are disjoint: at most m points)
    const int off = rs - (incl - rl);                             // candidate t of this lane's run is sorted[off + t]
    for (int t0 = 0; t0 < T; t0 += 64) {                          // wave-uniform
        const int t = t0 + lane;
        int j = 0;                                                // the run of candidate t: the number of lanes with incl <= t
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const int v = __shfl(incl, j + s - 1, 64);
            if (v <= t) j += s;
        }
        const int o = __shfl(off, j, 64);
        if (t < T) {
            const float4 v = sp[min(max(o + t, 0), m - 1)];        // (always inside: start[] ascends from 0 to m)
            tnn_insert(tnn_make_key(gad_sqdist(ux, uy, uz, v.x, v.y, v.z), __float_as_int(v.w)), k0, k1, k2);
        }
    }
}

// one axis of the stop test, in cells: `face` = the query's distance to the nearest face of the block [i - r, i + r] that is not
// a border of the grid (+inf: none), `out` = its distance to the box (0 inside); f is the query's computed cell coordinate
__device__ __forceinline__ void tnn_axis(float f, int i, int r, int n, float& face, float& out) {
    const float fc = f != f ? 0.f : fminf(fmaxf(f, -2048.f), 3072.f);   // (NaN: an overflowed difference times inv = 0, one cell)
    face = __builtin_huge_valf();
    if (i - r > 0) face = fminf(face, fc - (float)(i - r));
    if (i + r < n - 1) face = fminf(face, (float)(i + r + 1) - fc);
    out = fmaxf(0.f, fmaxf(-fc, fc - (float)n));
}
__device__ __forceinline__ float tnn_sq_less_slack(float cells) {
    const float v = fmaxf(cells - TNN_CELL_SLACK, 0.f);
    return v * v;
}

__global__ __launch_bounds__(256) void tnn_query_kernel(const float* __restrict__ unknown, const float* __restrict__ known, int n,
                                                        int m, int per_wave, int cells, const PointGrid* __restrict__ hdr,
                                                        const int32_t* __restrict__ start, const float4* __restrict__ sorted,
                                                        float* __restrict__ dist2, int32_t* __restrict__ idx,
                                                        int32_t* __restrict__ stats) {
    const int b = blockIdx.y, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long long q0 = ((long long)blockIdx.x * 4 + wave) * per_wave;
    if (q0 >= n) return;                                          // wave-uniform; the kernel has no workgroup barrier
    const int q1 = (int)min((long long)n, q0 + per_wave);
    const PointGrid g = hdr[b];
    const int32_t* st = start + (size_t)b * (cells + 1);
    const float4* sp = sorted + (size_t)b * m;
    const float* kb = known + (size_t)b * m * 3;
    const float inf = __builtin_huge_valf();
    int from_grid = 0, redone = 0;
    for (int i = (int)q0; i < q1; ++i) {                          // wave-uniform
        const size_t o3 = ((size_t)b * n + i) * 3;
        const float ux = unknown[o3], uy = unknown[o3 + 1], uz = unknown[o3 + 2];
        tnn_key k0 = TNN_INF_KEY, k1 = TNN_INF_KEY, k2 = TNN_INF_KEY, g0 = TNN_INF_KEY, g1 = TNN_INF_KEY, g2 = TNN_INF_KEY;
        bool done = !(pg_finite(ux) && pg_finite(uy) && pg_finite(uz));
        if (!done) {
            const float fx = (ux - g.lox) * g.ivx, fy = (uy - g.loy) * g.ivy, fz = (uz - g.loz) * g.ivz;
            const int ix = pg_cell1(ux, g.lox, g.ivx, g.nx), iy = pg_cell1(uy, g.loy, g.ivy, g.ny), iz = pg_cell1(uz, g.loz, g.ivz, g.nz);
            for (int r = 1; r <= TNN_RINGS && !done; ++r) {
                // lane = one (y, z) row of the (2r + 1)^2 around the query's: on the shell's y / z faces (and in the first block)
                // the whole x run of the block, else its two end cells, one per pass
                const int side = 2 * r + 1;
                const int dy = lane % side - r, dz = lane / side - r, y = iy + dy, z = iz + dz;
                const bool row = lane < side * side && y >= 0 && y < g.ny && z >= 0 && z < g.nz;
                const bool whole = r == 1 || dy == r || dy == -r || dz == r || dz == -r;
                const int base = row ? (z * g.ny + y) * g.nx : 0;
                for (int pass = 0; pass < (r == 1 ? 1 : 2); ++pass) {
                    int x0 = 0, x1 = -1;                          // cells [x0, x1] of the row
                    if (row && whole && pass == 0) { x0 = max(ix - r, 0); x1 = min(ix + r, g.nx - 1); }
                    if (row && !whole && pass == 0 && ix - r >= 0) x0 = x1 = ix - r;
                    if (row && !whole && pass == 1 && ix + r <= g.nx - 1) x0 = x1 = ix + r;
                    int rs = 0, rl = 0;
                    if (x1 >= x0) {
                        rs = st[base + x0];
                        rl = st[base + x1 + 1] - rs;
                    }
                    tnn_scan_runs(sp, m, rs, max(rl, 0), lane, ux, uy, uz, k0, k1, k2);
                }
                tnn_wave_best3(k0, k1, k2, g0, g1, g2);
                float ax, ay, az, ox, oy, oz;
                tnn_axis(fx, ix, r, g.nx, ax, ox);
                tnn_axis(fy, iy, r, g.ny, ay, oy);
                tnn_axis(fz, iz, r, g.nz, az, oz);
                if (ax == inf && ay == inf && az == inf) {
                    done = true;                                  // the block covers the grid
                } else {
                    const float px = tnn_sq_less_slack(ox), py = tnn_sq_less_slack(oy), pz = tnn_sq_less_slack(oz);
                    float c2 = inf;                               // the least squared distance, in cells, beyond any such face
                    if (ax < inf) c2 = fminf(c2, tnn_sq_less_slack(ax) + (py + pz));
                    if (ay < inf) c2 = fminf(c2, tnn_sq_less_slack(ay) + (px + pz));
                    if (az < inf) c2 = fminf(c2, tnn_sq_less_slack(az) + (px + py));
                    const float L = sqrtf(c2) / g.ivx;
                    const float bound = L * L * 0.99999f;
                    done = bound > 1.0e-30f && __uint_as_float((unsigned)(g2 >> 32)) < bound;
                }
            }
            if (done) {
                ++from_grid;
            } else {                                              // the exhaustive walk, from empty lists
                ++redone;
                k0 = k1 = k2 = TNN_INF_KEY;
#pragma unroll 4
                for (int k = lane; k < m; k += 64)
                    tnn_insert(tnn_make_key(gad_sqdist(ux, uy, uz, kb[k * 3 + 0], kb[k * 3 + 1], kb[k * 3 + 2]), k), k0, k1, k2);
                tnn_wave_best3(k0, k1, k2, g0, g1, g2);
            }
        } else {
            ++from_grid;
        }
        if (lane < 3) {
            const tnn_key k = lane == 0 ? g0 : (lane == 1 ? g1 : g2);
            dist2[o3 + lane] = __uint_as_float((unsigned)(k >> 32));
            idx[o3 + lane] = (int32_t)(unsigned)k;
        }
    }
    if (stats && lane == 0) {                                     // at most one add per counter and wavefront
        if (from_grid) atomicAdd(stats + b * 2, from_grid);
        if (redone) atomicAdd(stats + b * 2 + 1, redone);
    }
}

__global__ __launch_bounds__(64) void tnn_stats_exhaustive_kernel(int B, int n, int32_t* __restrict__ stats) {
    for (int b = threadIdx.x; b < B; b += 64) { stats[b * 2] = 0; stats[b * 2 + 1] = n; }
}

// the shape checks of gad_three_nn_grid, then the grid's for a cloud of max(m, 1) known points
static int tnn_plan(const char* who, int B, int n, int m, PointGridPlan* pl) {
    GAD_REQUIRE(B >= 0 && n >= 0 && m >= 0, GAD_ERR_SHAPE, "%s: negative size (B=%d n=%d m=%d)", who, B, n, m);
    GAD_REQUIRE((long long)m * 3 < (1ll << 31) && (long long)B * m < (1ll << 31) && (long long)B * n < (1ll << 31) && B <= 65535,
                GAD_ERR_SHAPE, "%s: B=%d clouds of n=%d queries and m=%d known points overflows 32-bit indexing (or B > 65535)", who, B, n, m);
    GAD_REQUIRE(m >= 1 || (long long)B * n == 0, GAD_ERR_SHAPE, "%s: no known point (m=%d) for n=%d queries", who, m, n);
    return point_grid_plan(who, B, std::max(m, 1), pl);
}

extern "C" long long gad_three_nn_grid_workspace_bytes(int B, int n, int m) {
    PointGridPlan pl;
    const int rc = tnn_plan("three_nn_grid_workspace_bytes", B, n, m, &pl);
    return rc != GAD_OK ? rc : pl.total;
}

extern "C" int gad_three_nn_grid(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx,
                                 int32_t* stats, void* workspace, void* stream) {
    GAD_REQUIRE(unknown && known && dist2 && idx, GAD_ERR_NULL, "three_nn_grid: null pointer (unknown / known / dist2 / idx)");
    PointGridPlan pl;
    int rc = tnn_plan("three_nn_grid", B, n, m, &pl);
    if (rc != GAD_OK) return rc;
    if ((long long)B * n == 0) return GAD_OK;
    PointGridView v;
    rc = point_grid_carve("three_nn_grid", workspace, pl, &v);
    if (rc != GAD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!g_geo_opt.tnn_grid) {
        const int tiles = gad_cdiv(n, 256);
        hipLaunchKernelGGL(three_nn_kernel, dim3(B * tiles), dim3(256), 0, st, unknown, known, n, m, tiles, dist2, idx);
        if (stats) hipLaunchKernelGGL(tnn_stats_exhaustive_kernel, dim3(1), dim3(64), 0, st, B, n, stats);
        GAD_CHECK_LAUNCH("three_nn_grid(exhaustive)");
        return GAD_OK;
    }
    // a wavefront takes a run of per_wave queries of one cloud: about TNN_WAVES_TARGET wavefronts, one query each below that
    const int per_wave = (int)std::max<long long>(1, gad_cdiv((long long)B * n, TNN_WAVES_TARGET));
    point_grid_build(known, B, m, pl, v, PG_EDGE_BUDGET, 0.f, stats, st);
    hipLaunchKernelGGL(tnn_query_kernel, dim3(gad_cdiv(gad_cdiv(n, per_wave), 4), B), dim3(256), 0, st, unknown, known, n, m, per_wave,
                       pl.cells, v.hdr, v.start, v.sorted, dist2, idx, stats);
    GAD_CHECK_LAUNCH("three_nn_grid");
    return GAD_OK;
}

// Consecutive lanes take consecutive points i (coalesced idx / weight reads and out writes); a lane reads its three indices and
// weights once and walks a chunk of TI_CH channels.  Workgroup = (point tile, channel chunk, sample), flattened into blockIdx.x.
#define TI_CH 8
__global__ __launch_bounds__(256) void three_interpolate_kernel(const float* __restrict__ pts, const int32_t* __restrict__ idx,
                                                                const float* __restrict__ w, int C, int m, int n, int tiles,
                                                                int chunks, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int tile = blockIdx.x % tiles, rest = blockIdx.x / tiles;
    const int c0 = (rest % chunks) * TI_CH, b = rest / chunks;
    const int i = tile * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t q = ((size_t)b * n + i) * 3;
    const int j0 = idx[q], j1 = idx[q + 1], j2 = idx[q + 2];
    const float w0 = w[q], w1 = w[q + 1], w2 = w[q + 2];
    const int c1 = min(c0 + TI_CH, C);
#pragma unroll 4
    for (int c = c0; c < c1; ++c) {
        const float* f = pts + ((size_t)b * C + c) * m;
        const float a0 = w0 * f[j0], a1 = w1 * f[j1], a2 = w2 * f[j2];
        out[((size_t)b * C + c) * n + i] = (a0 + a1) + a2;
    }
}

__global__ __launch_bounds__(256) void three_interpolate_grad_kernel(const float* __restrict__ go, const int32_t* __restrict__ idx,
                                                                     const float* __restrict__ w, int C, int n, int m, int tiles,
                                                                     int chunks, float* __restrict__ gp) {
    const int tile = blockIdx.x % tiles, rest = blockIdx.x / tiles;
    const int c0 = (rest % chunks) * TI_CH, b = rest / chunks;
    const int i = tile * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t q = ((size_t)b * n + i) * 3;
    const int j0 = idx[q], j1 = idx[q + 1], j2 = idx[q + 2];
    const float w0 = w[q], w1 = w[q + 1], w2 = w[q + 2];
    const int c1 = min(c0 + TI_CH, C);
#pragma unroll 4
    for (int c = c0; c < c1; ++c) {
        const float g = go[((size_t)b * C + c) * n + i];
        float* d = gp + ((size_t)b * C + c) * m;
        atomic_add_f32(d + j0, g * w0);
        atomic_add_f32(d + j1, g * w1);
        atomic_add_f32(d + j2, g * w2);
    }
}

// m <= TIG_NT: one workgroup per (sample, chunk of ch channels, ch * m <= TIG_NT) keeps its rows of grad_points in LDS, adds the
// entries of all n points with LDS atomics and stores the rows once -- no clearing pass, no global atomic (64 lanes scattering
// into a row with global atomics ran 1.2x slower than torch's own scatter at B 64, C 128, n 4096, m 1024).
#define TIG_NT 8192
__global__ __launch_bounds__(256) void three_interpolate_grad_lds_kernel(const float* __restrict__ go, const int32_t* __restrict__ idx,
                                                                         const float* __restrict__ w, int C, int n, int m, int ch,
                                                                         int chunks, float* __restrict__ gp) {
    __shared__ float acc[TIG_NT];
    const int b = blockIdx.x / chunks, c0 = (blockIdx.x - b * chunks) * ch, t = threadIdx.x;
    const int nc = min(ch, C - c0);
    for (int j = t; j < nc * m; j += 256) acc[j] = 0.f;
    __syncthreads();
    for (long long i = t; i < n; i += 256) {
        const size_t q = ((size_t)b * n + i) * 3;
        const int j0 = idx[q], j1 = idx[q + 1], j2 = idx[q + 2];
        const float w0 = w[q], w1 = w[q + 1], w2 = w[q + 2];
        for (int c = 0; c < nc; ++c) {
            const float g = go[((size_t)b * C + c0 + c) * n + i];
            float* d = acc + c * m;
            atomic_add_f32(d + j0, g * w0);
            atomic_add_f32(d + j1, g * w1);
            atomic_add_f32(d + j2, g * w2);
        }
    }
    __syncthreads();
    float* dst = gp + ((size_t)b * C + c0) * m;          // the chunk's rows are contiguous
    for (int j = t; j < nc * m; j += 256) dst[j] = acc[j];
}

// (tiles, chunks) of the flattened (point tile, channel chunk, sample) grid; false with the error set if it does not fit
static bool ti_grid(const char* what, int B, int C, int n, int* tiles, int* chunks) {
    *tiles = gad_cdiv(n, 256);
    *chunks = gad_cdiv(C, TI_CH);
    if ((long long)B * *tiles * *chunks < (1ll << 31)) return true;
    gad_set_error("%s: B * C * n too large", what);
    return false;
}

extern "C" int gad_three_interpolate(const float* points, const int32_t* idx, const float* weight, int B, int C, int m, int n,
                                     float* out, void* stream) {
    GAD_REQUIRE(points && idx && weight && out, GAD_ERR_NULL, "three_interpolate: null pointer");
    GAD_REQUIRE(B >= 0 && C >= 0 && m >= 0 && n >= 0, GAD_ERR_SHAPE, "three_interpolate: negative size (B %d, C %d, m %d, n %d)", B,
                C, m, n);
    if ((long long)B * C * n == 0) return GAD_OK;
    GAD_REQUIRE(m >= 1, GAD_ERR_SHAPE, "three_interpolate: no known point (m = %d) for %d points", m, n);
    int tiles, chunks;
    if (!ti_grid("three_interpolate", B, C, n, &tiles, &chunks)) return GAD_ERR_SHAPE;
    hipLaunchKernelGGL(three_interpolate_kernel, dim3(B * tiles * chunks), dim3(256), 0, (hipStream_t)stream, points, idx, weight, C,
                       m, n, tiles, chunks, out);
    GAD_CHECK_LAUNCH("three_interpolate");
    return GAD_OK;
}

extern "C" int gad_three_interpolate_grad(const float* grad_out, const int32_t* idx, const float* weight, int B, int C, int n, int m,
                                          float* grad_points, void* stream) {
    GAD_REQUIRE(grad_out && idx && weight && grad_points, GAD_ERR_NULL, "three_interpolate_grad: null pointer");
    GAD_REQUIRE(B >= 0 && C >= 0 && m >= 0 && n >= 0, GAD_ERR_SHAPE, "three_interpolate_grad: negative size (B %d, C %d, n %d, m %d)",
                B, C, n, m);
    GAD_REQUIRE(m >= 1 || (long long)B * C * n == 0, GAD_ERR_SHAPE, "three_interpolate_grad: no known point (m = %d) for %d points", m, n);
    if ((long long)B * C * m == 0) return GAD_OK;
    hipStream_t st = (hipStream_t)stream;
    if (gad_deterministic()) {                           // (writes every element of grad_points: no clearing pass)
        GAD_REQUIRE((long long)B * C < (1ll << 31) && (long long)n * 3 < (1ll << 31), GAD_ERR_SHAPE,
                    "three_interpolate_grad: B * C or 3 * n too large");
        group_points_grad_weighted_launch(grad_out, idx, weight, B, C, m, n * 3, grad_points, st);      // group.hip's ordered scatter
        GAD_CHECK_LAUNCH("three_interpolate_grad");
        return GAD_OK;
    }
    if (m <= TIG_NT) {
        const int ch = min(TI_CH, TIG_NT / m), cch = gad_cdiv(C, ch);
        GAD_REQUIRE((long long)B * cch < (1ll << 31), GAD_ERR_SHAPE, "three_interpolate_grad: B * C too large");
        hipLaunchKernelGGL(three_interpolate_grad_lds_kernel, dim3(B * cch), dim3(256), 0, st, grad_out, idx, weight, C, n, m, ch, cch,
                           grad_points);
        GAD_CHECK_LAUNCH("three_interpolate_grad");
        return GAD_OK;
    }
    int tiles, chunks;
    if (!ti_grid("three_interpolate_grad", B, C, n, &tiles, &chunks)) return GAD_ERR_SHAPE;
    { hipError_t me = hipMemsetAsync(grad_points, 0, sizeof(float) * (size_t)B * C * m, st); (void)me; }
    if (n == 0) return GAD_OK;
    hipLaunchKernelGGL(three_interpolate_grad_kernel, dim3(B * tiles * chunks), dim3(256), 0, st, grad_out, idx, weight, C, n, m, tiles,
                       chunks, grad_points);
    GAD_CHECK_LAUNCH("three_interpolate_grad");
    return GAD_OK;
}
