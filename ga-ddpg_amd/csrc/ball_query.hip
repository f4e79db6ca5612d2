// Ball query in its four forms (wavefront scan, LDS-tiled, cell list in LDS, point grid in global memory) and query_and_group,
// which shares the first three: gad_ball_query, gad_ball_query_grid, gad_query_and_group.  Replaces upstream ball_query_gpu.cu.
#include "common.hpp"
#include "point_grid.hpp"

// ------------------------------------------------------------------------------------------------
// ball query: one wavefront per centroid, ballot + prefix popcount keeps ascending index order
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_ball_query(const float* __restrict__ p, int N, float cx, float cy,
                                               float cz, float r2, int nsample, int lane,
                                               int32_t* __restrict__ out) {
    int cnt = 0, first = 0;
    for (int base = 0; base < N && cnt < nsample; base += 64) {
        const int k = base + lane;
        bool in = false;
        if (k < N) {
            const float d2 = gad_sqdist(cx, cy, cz, p[k * 3 + 0], p[k * 3 + 1], p[k * 3 + 2]);
            in = d2 < r2;
        }
        const unsigned long long mask = __ballot(in);
        if (mask) {
            if (cnt == 0) first = base + __ffsll((long long)mask) - 1;
            const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
            if (in && slot < nsample) out[slot] = k;
            cnt += __popcll(mask);
        }
    }
    cnt = cnt < nsample ? cnt : nsample;
    for (int s = cnt + lane; s < nsample; s += 64) out[s] = first;   // pad with the first hit (0 if none)
    return cnt;
}

// Radius search for LARGE clouds (N > 1024: BASELINE configs[3], 512 centroids x 4096 points x 128 clouds = 2.7e8
// distance tests).  The one-wavefront-per-centroid scan above is bound by VALU issue: ~15 instructions per 64 tests,
// each lane re-loading its point for every centroid.  Here a workgroup stages its cloud once in LDS (structure of
// arrays) and every wavefront scans it for SIXTEEN centroids at a time, two per packed instruction (v_pk_add/mul_f32
// keep the pinned evaluation order ((dx*dx)+(dy*dy))+(dz*dz) with every operation rounded: fp contraction is off in
// this function), i.e. ~5 instructions per 64 tests instead of ~15.  Results are identical to the scan above (same
// predicate, same ascending compaction).  Measured at configs[3]: ball query 198 -> 134 us, query_and_group 224 -> 179 us;
// the floor of this brute-force formulation is ~40 us of packed arithmetic (a cell list was the next step: in LDS below for
// N <= BQ_MAXN, in global memory -- gad_ball_query_grid -- for larger clouds).
typedef float gad_f32x2 __attribute__((ext_vector_type(2)));
#define BQ_CPW 16                                  // centroids per wavefront
#define BQ_MAXN 4096                               // points staged in LDS (48 KB)

__device__ __forceinline__ gad_f32x2 bq_sqdist2(gad_f32x2 cx, gad_f32x2 cy, gad_f32x2 cz, float x, float y, float z) {
#pragma clang fp contract(off)
    const gad_f32x2 dx = cx - gad_f32x2{x, x}, dy = cy - gad_f32x2{y, y}, dz = cz - gad_f32x2{z, z};
    const gad_f32x2 xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

// idx rows + counts of the 4 * BQ_CPW centroids [m0, m0 + 4 * BQ_CPW) of one cloud; lists: LDS, 4 * BQ_CPW x nsample ints
__device__ __forceinline__ void bq_tile_scan(const float* __restrict__ xs, const float* __restrict__ ys,
                                             const float* __restrict__ zs, int N, const float* __restrict__ ctr, int m0,
                                             int M, float r2, int nsample, int32_t* __restrict__ lists,
                                             int (&cnt)[BQ_CPW]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    gad_f32x2 cx[BQ_CPW / 2], cy[BQ_CPW / 2], cz[BQ_CPW / 2];
    int first[BQ_CPW];
#pragma unroll
    for (int j = 0; j < BQ_CPW; ++j) {
        const int m = min(m0 + wave * BQ_CPW + j, M - 1);        // clamped: surplus slots repeat the last centroid, not written
        const float* c = ctr + (size_t)m * 3;
        cx[j >> 1][j & 1] = c[0]; cy[j >> 1][j & 1] = c[1]; cz[j >> 1][j & 1] = c[2];
        cnt[j] = 0; first[j] = 0;
    }
    for (int base = 0; base < N; base += 64) {
        const int k = base + lane;
        const bool live = k < N;
        // lanes past the end of the cloud get a far-away point: the plain predicate d2 < r2 is then false for them and the
        // ballot is a single v_cmp (no extra masking per centroid)
        const float x = live ? xs[k] : 3.0e18f, y = live ? ys[k] : 3.0e18f, z = live ? zs[k] : 3.0e18f;
#pragma unroll
        for (int p = 0; p < BQ_CPW / 2; ++p) {
            const gad_f32x2 d2 = bq_sqdist2(cx[p], cy[p], cz[p], x, y, z);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int j = 2 * p + e;
                const bool in = d2[e] < r2;
                const unsigned long long mask = __ballot(in);
                if (mask) {                                   // wave-uniform; ~3 of 4 (centroid, chunk) pairs have no hit
                    if (cnt[j] == 0) first[j] = base + __ffsll((long long)mask) - 1;
                    const int slot = cnt[j] + __popcll(mask & ((1ull << lane) - 1ull));
                    if (in && slot < nsample) lists[(wave * BQ_CPW + j) * nsample + slot] = k;
                    cnt[j] += __popcll(mask);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < BQ_CPW; ++j) {
        cnt[j] = cnt[j] < nsample ? cnt[j] : nsample;
        for (int s2 = cnt[j] + lane; s2 < nsample; s2 += 64) lists[(wave * BQ_CPW + j) * nsample + s2] = first[j];
    }
}

// mode 0: ball query only (idx, cnt);  mode 1: QueryAndGroup(use_xyz=True) output as well
__global__ __launch_bounds__(256) void ball_query_tiled_kernel(const float* __restrict__ new_xyz,
                                                               const float* __restrict__ xyz,
                                                               const float* __restrict__ feat, int C, int N, int M,
                                                               float r2, int S, int32_t* __restrict__ idx,
                                                               int32_t* __restrict__ cnt_out, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float bq_lds[];
    float* xs = bq_lds;
    float* ys = xs + N;
    float* zs = ys + N;
    int32_t* lists = reinterpret_cast<int32_t*>(zs + N);          // (4 * BQ_CPW) x S
    const int b = blockIdx.y, m0 = blockIdx.x * 4 * BQ_CPW;
    const float* p = xyz + (size_t)b * N * 3;
    for (int i = threadIdx.x; i < N; i += 256) { xs[i] = p[i * 3 + 0]; ys[i] = p[i * 3 + 1]; zs[i] = p[i * 3 + 2]; }
    __syncthreads();
    int cnt[BQ_CPW];
    bq_tile_scan(xs, ys, zs, N, new_xyz + (size_t)b * M * 3, m0, M, r2, S, lists, cnt);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");        // a wavefront reads back only its own lists
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t plane = (size_t)M * S;
#pragma unroll
    for (int j = 0; j < BQ_CPW; ++j) {
        const int m = m0 + wave * BQ_CPW + j;
        if (m >= M) break;                                        // wave-uniform
        const size_t g = (size_t)b * M + m;
        const int32_t* my = lists + (wave * BQ_CPW + j) * S;
        if (lane == 0 && cnt_out) cnt_out[g] = cnt[j];
        const float* c = new_xyz + g * 3;
        const float ccx = c[0], ccy = c[1], ccz = c[2];
        float* o = out ? out + ((size_t)b * (3 + C)) * plane + (size_t)m * S : nullptr;
        for (int s2 = lane; s2 < S; s2 += 64) {
            const int k = my[s2];
            idx[g * S + s2] = k;
            if (o) {
                o[0 * plane + s2] = __fsub_rn(xs[k], ccx);
                o[1 * plane + s2] = __fsub_rn(ys[k], ccy);
                o[2 * plane + s2] = __fsub_rn(zs[k], ccz);
                const float* f = feat + (size_t)b * C * N + k;
                for (int ch = 0; ch < C; ++ch) o[(3 + ch) * plane + s2] = f[(size_t)ch * N];
            }
        }
    }
}

// ---- cell-list radius search (configs[3] regime: thousands of points, a radius that is a small fraction of the cloud) ----
// The brute-force tile scan above tests every (centroid, point) pair: 4096 tests per centroid at configs[3] for ~17 hits.
// Here one 1024-thread workgroup sorts its cloud ONCE into a uniform grid held in LDS (cell edge >= 1.001 x radius, so
// every in-radius point lies in the 3x3x3 cells around the centroid's cell: ~110 candidates), then each wavefront takes
// four centroids at a time (16 lanes each): the candidates of the nine (y,z) cell rows -- three x-adjacent cells are one
// contiguous run of the sorted cloud -- get the exact pinned-order distance test, and hits set bit k of the centroid's
// N-bit LDS bitmap.  The bitmap is then read back in ASCENDING point order (one 64-bit word per lane, popcount prefix
// scan), which is the reference's result order (first nsample hits by index) whatever order the cells were visited in:
// indices, counts and the grouped tensor are bit-identical to the scans above.  Cells are only an acceleration
// structure: a centroid outside the cloud's bounding box is clamped to the border cell, which still covers every
// candidate it can have, and the exact predicate d2 < r2 decides.
#define BQC_THREADS 1024
#define BQC_WAVES 16
#define BQC_GMAX 12                                // cells per axis; 12^3 = 1728
#define BQC_MAXCELLS 1728
#define BQC_MB 256                                 // centroids per workgroup

struct BqcGrid { float lox, loy, loz, ivx, ivy, ivz; int nx, ny, nz; };

// cells along one axis: edge >= h (= 1.001 r).  Only an acceleration structure, so approximate arithmetic is fine as
// long as the edge never drops below the radius: the 1e-3 (1e-4) slack covers the ~1e-7 error of v_rcp_f32
__device__ __forceinline__ int bqc_axis(float lo, float hi, float inv_h, float& inv) {
    const float ext = hi - lo;
    int n = (int)(ext * inv_h) + 1;
    inv = inv_h;
    if (!(n <= BQC_GMAX)) { n = BQC_GMAX; inv = (float)BQC_GMAX * __builtin_amdgcn_rcpf(ext * 1.0001f); }   // coarser cells
    return n < 1 ? 1 : n;
}
__device__ __forceinline__ int bqc_cell1(float p, float lo, float inv, int n) {
    const int c = (int)floorf((p - lo) * inv);
    return c < 0 ? 0 : (c >= n ? n - 1 : c);
}

// DPP cross-lane helpers (row = 16 lanes): no LDS traffic, unlike __shfl (ds_bpermute)
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_i(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false); }
__device__ __forceinline__ int row_incl_scan(int x) {             // inclusive prefix sum inside each 16-lane row
    x += dpp_i<0x111>(0, x); x += dpp_i<0x112>(0, x); x += dpp_i<0x114>(0, x); x += dpp_i<0x118>(0, x);   // row_shr:1,2,4,8
    return x;
}
__device__ __forceinline__ int wave_incl_scan(int x) {            // inclusive prefix sum over the wavefront
    x = row_incl_scan(x);
    x += dpp_i<0x142, 0xa>(0, x);                                  // row_bcast:15 -> rows 1, 3
    x += dpp_i<0x143, 0xc>(0, x);                                  // row_bcast:31 -> rows 2, 3
    return x;
}
__device__ __forceinline__ float row_max_f(float v) {             // lane 15 of each row: the row maximum
    v = fmaxf(v, __int_as_float(dpp_i<0x111>(__float_as_int(v), __float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_i<0x112>(__float_as_int(v), __float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_i<0x114>(__float_as_int(v), __float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_i<0x118>(__float_as_int(v), __float_as_int(v))));
    return v;
}
__device__ __forceinline__ float wave_max_f(float v) {            // every lane gets the wavefront maximum
    const int i = __float_as_int(row_max_f(v));
    return fmaxf(fmaxf(__int_as_float(__builtin_amdgcn_readlane(i, 15)), __int_as_float(__builtin_amdgcn_readlane(i, 31))),
                 fmaxf(__int_as_float(__builtin_amdgcn_readlane(i, 47)), __int_as_float(__builtin_amdgcn_readlane(i, 63))));
}

#define BQC_QUADS (BQC_MB / (4 * BQC_WAVES))       // passes of four centroids per wavefront
#define BQC_CPIPE 4                                // feature channels the grouped-output phase keeps in flight per lane
// LDS map (bytes; the cloud arrays are sized for BQ_MAXN so that every offset is an instruction immediate)
#define BQC_L_SY 16384
#define BQC_L_SZ 32768
#define BQC_L_SIDX 49152                           // u16[4096]  sorted slot -> point index
#define BQC_L_SPOS 57344                           // u16[4096]  point index -> sorted slot
#define BQC_L_BM 65536                             // u64[waves][4][64]  per-centroid bitmaps
#define BQC_L_TAB 98304                            // u32[waves][16][9]  (candidate run: first sorted slot | length << 16)
#define BQC_L_CSTART 107520                        // i32[BQC_MAXCELLS + 4]
#define BQC_L_RED 114448                           // f32[128]
#define BQC_L_LISTS 114960                         // i32[waves][4][SP]; the build's scatter cursors live here first

// SP: list stride (nsample <= SP).  The workgroup's 256 centroids: wavefront w takes quads q = w + 16 qi (qi < 4) of
// four consecutive centroids; lane group sub = lane / 16 works on centroid 4q + sub.
template <int SP>
__global__ __launch_bounds__(BQC_THREADS) void ball_query_cells_kernel(const float* __restrict__ new_xyz,
                                                                       const float* __restrict__ xyz,
                                                                       const float* __restrict__ feat, int C, int N, int M,
                                                                       float radius, int S, int32_t* __restrict__ idx,
                                                                       int32_t* __restrict__ cnt_out, float* __restrict__ out, int dbg) {
    extern __shared__ __attribute__((aligned(16))) float bq_lds[];
    char* const L = reinterpret_cast<char*>(bq_lds);
    float* const sx = reinterpret_cast<float*>(L);
    float* const sy = reinterpret_cast<float*>(L + BQC_L_SY);
    float* const sz = reinterpret_cast<float*>(L + BQC_L_SZ);
    unsigned short* const sidx = reinterpret_cast<unsigned short*>(L + BQC_L_SIDX);
    unsigned short* const spos = reinterpret_cast<unsigned short*>(L + BQC_L_SPOS);
    unsigned long long* const bm = reinterpret_cast<unsigned long long*>(L + BQC_L_BM);
    unsigned* const tab = reinterpret_cast<unsigned*>(L + BQC_L_TAB);
    int32_t* const cstart = reinterpret_cast<int32_t*>(L + BQC_L_CSTART);
    float* const red = reinterpret_cast<float*>(L + BQC_L_RED);
    int32_t* const lists = reinterpret_cast<int32_t*>(L + BQC_L_LISTS);
    int32_t* const cursor = lists;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave: an SGPR
    const int sub = lane >> 4, l16 = lane & 15;
    const int b = blockIdx.y, m0 = blockIdx.x * BQC_MB;
    const int m_end = min(M, m0 + BQC_MB);
    const float* p = xyz + (size_t)b * N * 3;

    // lane c16 = lane % 16 prepares centroid 4 * (wave + 16 * (c16 / 4)) + c16 % 4 (the four lane rows in unison); its
    // coordinates are fetched now so that the latency hides behind the build
    const int pm = m0 + 4 * (wave + BQC_WAVES * (l16 >> 2)) + (l16 & 3);
    float pcx, pcy, pcz;
    {
        const float* c = new_xyz + ((size_t)b * M + min(pm, M - 1)) * 3;
        pcx = c[0]; pcy = c[1]; pcz = c[2];
    }
    if (dbg & 8) return;
    // ---- build: bounding box -> grid -> counting sort -------------------------------------------------------------
    float px[4], py[4], pz[4];
    float hi[6] = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};          // max of (x, y, z, -x, -y, -z)
    // thread t owns points 4t .. 4t+3: three 16-byte loads when the cloud is 16-byte aligned (N % 4 == 0)
    const bool vec = (N & 3) == 0 && (reinterpret_cast<size_t>(xyz) & 15) == 0;
    if (vec) {
        if (4 * tid < N) {
            const float4* p4 = reinterpret_cast<const float4*>(p) + 3 * tid;
            const float4 a = p4[0], bq = p4[1], cq = p4[2];
            px[0] = a.x; py[0] = a.y; pz[0] = a.z; px[1] = a.w; py[1] = bq.x; pz[1] = bq.y;
            px[2] = bq.z; py[2] = bq.w; pz[2] = cq.x; px[3] = cq.y; py[3] = cq.z; pz[3] = cq.w;
        }
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = 4 * tid + u;
            if (k < N) { px[u] = p[k * 3 + 0]; py[u] = p[k * 3 + 1]; pz[u] = p[k * 3 + 2]; }
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (4 * tid + u < N) {
            hi[0] = fmaxf(hi[0], px[u]); hi[1] = fmaxf(hi[1], py[u]); hi[2] = fmaxf(hi[2], pz[u]);
            hi[3] = fmaxf(hi[3], -px[u]); hi[4] = fmaxf(hi[4], -py[u]); hi[5] = fmaxf(hi[5], -pz[u]);
        }
    }
    for (int c = tid; c < BQC_MAXCELLS + 4; c += BQC_THREADS) cstart[c] = 0;
    for (int i = tid; i < BQC_WAVES * 4 * 64; i += BQC_THREADS) bm[i] = 0ull;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        hi[a] = wave_max_f(hi[a]);
        if (lane == 0) red[a * BQC_WAVES + wave] = hi[a];
    }
    __syncthreads();
    if (dbg & 16) return;
#pragma unroll
    for (int a = 0; a < 6; ++a)                                    // 16 per-wavefront values = one lane row
        hi[a] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(row_max_f(red[a * BQC_WAVES + l16])), 15));
    BqcGrid g;
    const float inv_h = __builtin_amdgcn_rcpf(radius * 1.001f);
    g.lox = -hi[3]; g.loy = -hi[4]; g.loz = -hi[5];
    g.nx = bqc_axis(g.lox, hi[0], inv_h, g.ivx);
    g.ny = bqc_axis(g.loy, hi[1], inv_h, g.ivy);
    g.nz = bqc_axis(g.loz, hi[2], inv_h, g.ivz);
    const int ncell = g.nx * g.ny * g.nz;

    int cell[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k = 4 * tid + u;
        cell[u] = 0;
        if (k < N) {
            cell[u] = (bqc_cell1(pz[u], g.loz, g.ivz, g.nz) * g.ny + bqc_cell1(py[u], g.loy, g.ivy, g.ny)) * g.nx +
                      bqc_cell1(px[u], g.lox, g.ivx, g.nx);
            atomicAdd(&cstart[cell[u] + 1], 1);
        }
    }
    __syncthreads();
    if (dbg & 32) return;
    {   // inclusive scan of cstart[0 .. ncell] in place: two entries per thread (2048 >= BQC_MAXCELLS + 1)
        int32_t* wtot = reinterpret_cast<int32_t*>(red) + 6 * BQC_WAVES;
        const int e0 = 2 * tid;
        const int2 a = *reinterpret_cast<const int2*>(cstart + min(e0, BQC_MAXCELLS + 2));
        const int a0 = e0 <= ncell ? a.x : 0, a1 = e0 + 1 <= ncell ? a.y : 0;
        const int incl = wave_incl_scan(a0 + a1);
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        const int winc = row_incl_scan(wtot[l16]);                 // 16 wavefront totals = one lane row
        const int base = wave == 0 ? 0 : __shfl(winc, wave - 1, 64);
        const int excl = base + incl - (a0 + a1);
        if (e0 <= ncell) { cstart[e0] = excl + a0; cursor[e0] = excl + a0; }
        if (e0 + 1 <= ncell) { cstart[e0 + 1] = excl + a0 + a1; cursor[e0 + 1] = excl + a0 + a1; }
    }
    __syncthreads();
    if (dbg & 64) return;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k = 4 * tid + u;
        if (k < N) {
            const int t = atomicAdd(&cursor[cell[u]], 1);
            sx[t] = px[u]; sy[t] = py[u]; sz[t] = pz[u];
            sidx[t] = (unsigned short)k; spos[k] = (unsigned short)t;
        }
    }
    __syncthreads();

    // ---- candidate runs of this wavefront's 16 centroids: nine (y, z) cell rows, three x-adjacent cells = one run ----
    {
        const int cx = bqc_cell1(pcx, g.lox, g.ivx, g.nx), cy = bqc_cell1(pcy, g.loy, g.ivy, g.ny),
                  cz = bqc_cell1(pcz, g.loz, g.ivz, g.nz);
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1) + 1;
        const int nyx = g.ny * g.nx, rb0 = (cz * g.ny + cy) * g.nx;
        unsigned* te = tab + (wave * 16 + l16) * 9;
#pragma unroll
        for (int rr = 0; rr < 9; ++rr) {
            const int dy = (rr % 3) - 1, dz = (rr / 3) - 1;
            const bool ok = pm < m_end && (unsigned)(cy + dy) < (unsigned)g.ny && (unsigned)(cz + dz) < (unsigned)g.nz;
            const int rb = ok ? rb0 + dz * nyx + dy * g.nx : 0;
            const int beg = cstart[rb + x0], end = cstart[rb + x1];
            if (sub == 0) te[rr] = ok ? (unsigned)beg | ((unsigned)(end - beg) << 16) : 0u;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");         // from here on a wavefront touches only its own LDS rows
    __builtin_amdgcn_wave_barrier();

    // ---- query: four centroids per wavefront pass, 16 lanes each ----------------------------------------------------
    const float r2 = radius * radius;
    // the centroid of (pass qi, lane group sub) was prepared by lane 4 qi + sub
    float qx[BQC_QUADS], qy[BQC_QUADS], qz[BQC_QUADS];
#pragma unroll
    for (int qi = 0; qi < BQC_QUADS; ++qi) {
        qx[qi] = __shfl(pcx, 4 * qi + sub, 64); qy[qi] = __shfl(pcy, 4 * qi + sub, 64); qz[qi] = __shfl(pcz, 4 * qi + sub, 64);
    }
    const unsigned bmrow = BQC_L_BM + (unsigned)(wave * 4 + sub) * 512u;        // LDS byte address of this lane group's bitmap
    unsigned long long* const bw = bm + (size_t)(wave * 4 + sub) * 64;
    int32_t* const mylist = lists + (size_t)(wave * 4 + sub) * SP;
    const size_t plane = (size_t)M * S;
    const bool pipe = SP == 64 && C <= BQC_CPIPE;
    float pf[4][BQC_CPIPE];
    int pend_q = -1;
    // candidate slot t of the sorted cloud: exact test, hit -> bit k of the bitmap (a miss ORs in 0; slots past the end of a
    // run read whatever follows -- in bounds of the LDS allocation -- and are masked by `valid`)
    auto mark = [&](unsigned k, bool hit) {
        atomicOr(reinterpret_cast<unsigned*>(L + (bmrow | ((k >> 3) & 0x1fcu))), hit ? 1u << (k & 31) : 0u);
    };
    auto probe = [&](unsigned t, bool valid, float ccx, float ccy, float ccz) {
        const float x = sx[t], y = sy[t], z = sz[t];
        const unsigned k = sidx[t];
        mark(k, valid & (gad_sqdist(ccx, ccy, ccz, x, y, z) < r2));
    };
#pragma unroll
    for (int qi = 0; qi < BQC_QUADS; ++qi) {
        const int q = wave + qi * BQC_WAVES;
        if (m0 + 4 * q >= m_end) break;                            // wave-uniform
        const float ccx = qx[qi], ccy = qy[qi], ccz = qz[qi];
        if (!(dbg & 2)) {
            const unsigned* te = tab + (wave * 16 + qi * 4 + sub) * 9;
            const unsigned short* te16 = reinterpret_cast<const unsigned short*>(te);
            unsigned beg[9], len[9];
#pragma unroll
            for (int rr = 0; rr < 9; ++rr) { beg[rr] = te16[2 * rr]; len[rr] = te16[2 * rr + 1]; }
            // the first 16 slots of all nine runs (a run holds ~12 candidates at configs[3]): every LDS read is issued
            // before the first bitmap atomic, which the compiler will not move loads across
            float tx[9], ty[9], tz[9];
            unsigned tk[9];
#pragma unroll
            for (int rr = 0; rr < 9; ++rr) {
                const unsigned t = beg[rr] + (unsigned)l16;
                tx[rr] = sx[t]; ty[rr] = sy[t]; tz[rr] = sz[t]; tk[rr] = sidx[t];
            }
#pragma unroll
            for (int rr = 0; rr < 9; ++rr)
                mark(tk[rr], ((unsigned)l16 < len[rr]) & (gad_sqdist(ccx, ccy, ccz, tx[rr], ty[rr], tz[rr]) < r2));
#pragma unroll
            for (int rr = 0; rr < 9; ++rr) {
                if (__builtin_amdgcn_ballot_w64(len[rr] > 16u) != 0ull)                // wave-uniform
                    for (unsigned off = 16; __builtin_amdgcn_ballot_w64(off < len[rr]) != 0ull; off += 16)
                        probe(beg[rr] + (unsigned)l16 + off, off + (unsigned)l16 < len[rr], ccx, ccy, ccz);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (dbg & 4) continue;

        // ---- bitmaps -> ascending index lists, the four centroids side by side: lane l16 owns bits [256 l16, 256 l16 + 256)
        unsigned long long w[4];
        {
            const ulonglong2 w01 = *reinterpret_cast<const ulonglong2*>(bw + 4 * l16);
            const ulonglong2 w23 = *reinterpret_cast<const ulonglong2*>(bw + 4 * l16 + 2);
            w[0] = w01.x; w[1] = w01.y; w[2] = w23.x; w[3] = w23.y;
            *reinterpret_cast<ulonglong2*>(bw + 4 * l16) = ulonglong2{0ull, 0ull};
            *reinterpret_cast<ulonglong2*>(bw + 4 * l16 + 2) = ulonglong2{0ull, 0ull};
        }
        const int nb = __popcll(w[0]) + __popcll(w[1]) + __popcll(w[2]) + __popcll(w[3]);
        const int incl = row_incl_scan(nb);
        const int total = __shfl(incl, lane | 15, 64);
        int pos = incl - nb;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned long long ww = w[i];
            while (ww != 0ull && pos < S) {
                mylist[pos++] = 256 * l16 + 64 * i + (__ffsll((long long)ww) - 1);
                ww &= ww - 1ull;
            }
        }
        const int cnt = total < S ? total : S;
        if (cnt < S) {                                             // pad with the first hit (0 if the ball is empty)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const int first = total > 0 ? mylist[0] : 0;
            for (int s2 = cnt + l16; s2 < S; s2 += 16) mylist[s2] = first;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // ---- write-out: one centroid per 64-lane sweep.  Fast path (nsample <= 64, <= BQC_CPIPE feature channels): the
        // feature loads of this pass stay in flight across the NEXT pass's scan and are stored after it
        if (cnt_out && l16 == 0 && m0 + 4 * q + sub < m_end) cnt_out[(size_t)b * M + m0 + 4 * q + sub] = cnt;
        if (pipe) {
            const bool act = lane < S;
            if (out && pend_q >= 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {                      // phase C of the previous pass
                    const int mj = m0 + 4 * pend_q + j;            // uniform
                    float* oc = out + ((size_t)b * (3 + C) + 3) * plane + (size_t)mj * S;
                    if (mj < m_end) {
#pragma unroll
                        for (int ch = 0; ch < BQC_CPIPE; ++ch) {
                            if (ch < C && act) oc[lane] = pf[j][ch];
                            oc += plane;
                        }
                    }
                }
            }
            unsigned kk[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                          // phase A: indices and the feature loads of all four
                const bool okj = act && (m0 + 4 * q + j < m_end);
                kk[j] = okj ? (unsigned)(lists + (size_t)(wave * 4 + j) * SP)[lane] : 0u;
                if (out) {
                    const float* fc = feat + (size_t)b * C * N;
#pragma unroll
                    for (int ch = 0; ch < BQC_CPIPE; ++ch) {
                        if (ch < C) pf[j][ch] = fc[kk[j]];
                        fc += N;
                    }
                }
            }
            pend_q = q;
#pragma unroll
            for (int j = 0; j < 4; ++j) {                          // phase B: indices + recentred coordinates (LDS only)
                const int mj = m0 + 4 * q + j;
                if (mj >= m_end) break;
                const size_t gi = (size_t)b * M + mj;
                if (act) {
                    (idx + gi * S)[lane] = (int)kk[j];
                    if (out) {
                        const float jx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ccx), 16 * j));
                        const float jy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ccy), 16 * j));
                        const float jz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ccz), 16 * j));
                        float* orow = out + ((size_t)b * (3 + C)) * plane + (size_t)mj * S;
                        const unsigned t = spos[kk[j]];
                        orow[lane] = __fsub_rn(sx[t], jx);
                        (orow + plane)[lane] = __fsub_rn(sy[t], jy);
                        (orow + 2 * plane)[lane] = __fsub_rn(sz[t], jz);
                    }
                }
            }
        } else {
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const int mj = m0 + 4 * q + j;
                if (mj >= m_end) break;
                const size_t gi = (size_t)b * M + mj;
                const int32_t* my = lists + (size_t)(wave * 4 + j) * SP;
                const float jx = __shfl(ccx, 16 * j, 64), jy = __shfl(ccy, 16 * j, 64), jz = __shfl(ccz, 16 * j, 64);
                float* o = out ? out + ((size_t)b * (3 + C)) * plane + (size_t)mj * S : nullptr;
                for (int s2 = lane; s2 < S; s2 += 64) {
                    const int k = my[s2];
                    idx[gi * S + s2] = k;
                    if (o) {
                        const int t = spos[k];
                        o[0 * plane + s2] = __fsub_rn(sx[t], jx);
                        o[1 * plane + s2] = __fsub_rn(sy[t], jy);
                        o[2 * plane + s2] = __fsub_rn(sz[t], jz);
                        const float* f = feat + (size_t)b * C * N + k;
                        for (int ch = 0; ch < C; ++ch) o[(3 + ch) * plane + s2] = f[(size_t)ch * N];
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();                           // the lists are rewritten by the next pass
    }
    if (pipe && out && pend_q >= 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int mj = m0 + 4 * pend_q + j;
            float* oc = out + ((size_t)b * (3 + C) + 3) * plane + (size_t)mj * S;
            if (mj < m_end) {
#pragma unroll
                for (int ch = 0; ch < BQC_CPIPE; ++ch) {
                    if (ch < C && lane < S) oc[lane] = pf[j][ch];
                    oc += plane;
                }
            }
        }
    }
}

// where gad_ball_query and gad_query_and_group send a shape: the cell list, else the tiled kernel, else the caller's own scan kernel
enum BqRoute { BQ_CELLS, BQ_TILED, BQ_SCAN };
static BqRoute bq_route(int N, int nsample, float radius) {
    if (g_geo_opt.bq_cells && N > 1024 && N <= BQ_MAXN && radius > 0.f && radius < 1.0e18f && nsample <= 128) return BQ_CELLS;
    if (N > 1024 && N <= BQ_MAXN && nsample <= 256) return BQ_TILED;
    return BQ_SCAN;
}
// the launch of BQ_CELLS / BQ_TILED for either caller (gad_ball_query: feat and out null, C = 0), checked under names[r], the caller's
static int bq_launch(BqRoute r, const char* const* names, const float* new_xyz, const float* xyz, const float* feat, int B, int C, int N,
                     int M, float radius, int nsample, int32_t* idx, int32_t* cnt, float* out, hipStream_t st) {
    if (r == BQ_CELLS) {
        static bool attr_set = false;
        if (!attr_set) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ball_query_cells_kernel<64>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ball_query_cells_kernel<128>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            attr_set = true;
        }
        const dim3 grid(gad_cdiv(M, BQC_MB), B);
        if (nsample <= 64)
            hipLaunchKernelGGL(ball_query_cells_kernel<64>, grid, dim3(BQC_THREADS), BQC_L_LISTS + BQC_WAVES * 4 * 64 * 4, st, new_xyz,
                               xyz, feat, C, N, M, radius, nsample, idx, cnt, out, g_geo_opt.bq_cells);
        else
            hipLaunchKernelGGL(ball_query_cells_kernel<128>, grid, dim3(BQC_THREADS), BQC_L_LISTS + BQC_WAVES * 4 * 128 * 4, st, new_xyz,
                               xyz, feat, C, N, M, radius, nsample, idx, cnt, out, g_geo_opt.bq_cells);
    } else {
        const size_t lds = (size_t)3 * N * sizeof(float) + (size_t)4 * BQ_CPW * nsample * sizeof(int32_t);
        hipLaunchKernelGGL(ball_query_tiled_kernel, dim3(gad_cdiv(M, 4 * BQ_CPW), B), dim3(256), lds, st, new_xyz, xyz, feat, C, N, M,
                           radius * radius, nsample, idx, cnt, out);
    }
    GAD_CHECK_LAUNCH(names[r]);
    return GAD_OK;
}

__global__ __launch_bounds__(256) void ball_query_kernel(const float* __restrict__ new_xyz,
                                                         const float* __restrict__ xyz, int G, int N,
                                                         int M, float r2, int nsample,
                                                         int32_t* __restrict__ idx,
                                                         int32_t* __restrict__ cnt_out) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;
    const int lane = threadIdx.x & 63;
    const int b = g / M;
    const float* c = new_xyz + (size_t)g * 3;
    const int cnt = wave_ball_query(xyz + (size_t)b * N * 3, N, c[0], c[1], c[2], r2, nsample, lane,
                                    idx + (size_t)g * nsample);
    if (lane == 0 && cnt_out) cnt_out[g] = cnt;
}

extern "C" int gad_ball_query(const float* new_xyz, const float* xyz, int B, int N, int M, float radius,
                              int nsample, int32_t* idx, int32_t* cnt, void* stream) {
    GAD_REQUIRE(new_xyz && xyz && idx, GAD_ERR_NULL, "ball_query: null pointer");
    GAD_REQUIRE(B >= 0 && N >= 1 && M >= 0 && nsample >= 1, GAD_ERR_SHAPE, "ball_query: bad shape");
    const int G = B * M;
    if (G == 0) return GAD_OK;
    static const char* const names[] = {"ball_query(cells)", "ball_query(tiled)"};
    const BqRoute r = bq_route(N, nsample, radius);
    if (r != BQ_SCAN) return bq_launch(r, names, new_xyz, xyz, nullptr, B, 0, N, M, radius, nsample, idx, cnt, nullptr, (hipStream_t)stream);
    hipLaunchKernelGGL(ball_query_kernel, dim3(gad_cdiv(G, 4)), dim3(256), 0, (hipStream_t)stream, new_xyz,
                       xyz, G, N, M, radius * radius, nsample, idx, cnt);
    GAD_CHECK_LAUNCH("ball_query");
    return GAD_OK;
}

// ------------------------------------------------------------------------------------------------
// ball query of clouds beyond BQ_MAXN: a uniform grid per cloud in global memory (the caller's workspace)
// ------------------------------------------------------------------------------------------------
// Past BQ_MAXN points no workgroup can hold its cloud, and ball_query_kernel walks all N points for every centroid whose
// ball holds fewer than nsample of them -- the usual first-stage case.  Here every cloud is sorted once into a uniform grid
// (cell edge >= 1.002 x radius: every in-radius point lies in the 3x3x3 cells around the centroid's cell) and a wavefront
// tests only those cells' points.  Seven launches on the caller's stream, no host synchronisation, nothing sized by the data:
// the six of point_grid_build (point_grid.hip: bounds, setup with the edge taken from the radius, count, slices, scan, scatter), then
//   query    one wavefront per centroid: the nine (y, z) rows of three x-adjacent cells are nine contiguous runs of `sorted`;
//            every candidate gets the exact pinned-order predicate of the scan, hits are collected in LDS, and the nsample
//            smallest are placed by rank (number of smaller hit indices) -- the scan's ascending order whatever cell a
//            hit came from.  A centroid with more than BQG_HITS hits is redone by wave_ball_query in the same wavefront: exact,
//            and cheap in that regime because it stops at nsample hits.
// The grid only selects candidates.  Its cell function is monotone in the coordinate and clamped, so a centroid outside the box
// lands in a border cell that still has every candidate next to it; a non-finite coordinate maps to a valid cell and fails the
// predicate.  Rounding: (p - lo) * inv is off by < 1.3e-4 cells at PG_GMAX cells per axis, the edge has 2e-3 of slack.
#define BQG_HITS 512                               // hits of one centroid held in LDS

__global__ __launch_bounds__(256) void bqg_query_kernel(const float* __restrict__ new_xyz, const float* __restrict__ xyz, int G, int N,
                                                        int M, float r2, int nsample, int cells, const PointGrid* __restrict__ hdr,
                                                        const int32_t* __restrict__ start, const float4* __restrict__ sorted,
                                                        int32_t* __restrict__ idx, int32_t* __restrict__ cnt_out) {
    __shared__ int32_t hits[4][BQG_HITS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gi = blockIdx.x * 4 + wave;
    if (gi >= G) return;                                          // wave-uniform; the kernel has no workgroup barrier
    const int b = gi / M;
    const float* c = new_xyz + (size_t)gi * 3;
    const float cx = c[0], cy = c[1], cz = c[2];
    const PointGrid g = hdr[b];
    const int32_t* st = start + (size_t)b * (cells + 1);
    const float4* sp = sorted + (size_t)b * N;
    int32_t* out = idx + (size_t)gi * nsample;
    int32_t* my = hits[wave];
    const int ix = pg_cell1(cx, g.lox, g.ivx, g.nx), iy = pg_cell1(cy, g.loy, g.ivy, g.ny), iz = pg_cell1(cz, g.loz, g.ivz, g.nz);
    // lanes 0..8 take one (y, z) row each: its three x-adjacent cells are one run [rs, rs + rl) of the sorted cloud
    int rs = 0, rl = 0;
    if (lane < 9) {
        const int y = iy + lane % 3 - 1, z = iz + lane / 3 - 1;
        if (y >= 0 && y < g.ny && z >= 0 && z < g.nz) {
            const int row = (z * g.ny + y) * g.nx, x0 = max(ix - 1, 0), x1 = min(ix + 1, g.nx - 1);
            rs = st[row + x0];
            rl = st[row + x1 + 1] - rs;
        }
    }
    int incl = rl;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    int end[9], off[9];                                           // wave-uniform: candidate t of run j is sorted[off[j] + t]
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        end[j] = __shfl(incl, j, 64);
        off[j] = __shfl(rs, j, 64) - (end[j] - __shfl(rl, j, 64));
    }
    const int T = min(end[8], N);                                 // (the runs are disjoint: at most N candidates)
    const unsigned long long below = (1ull << lane) - 1ull;
    int H = 0;
    for (int t0 = 0; t0 < T && H <= BQG_HITS; t0 += 64) {
        const int t = t0 + lane;
        bool in = false;
        int k = 0;
        if (t < T) {
            int o = off[0];
#pragma unroll
            for (int j = 1; j < 9; ++j) o = t >= end[j - 1] ? off[j] : o;
            const float4 v = sp[min(max(o + t, 0), N - 1)];         // (always inside: start[] ascends from 0 to N)
            k = __float_as_int(v.w);
            in = gad_sqdist(cx, cy, cz, v.x, v.y, v.z) < r2;
        }
        const unsigned long long mask = __ballot(in);
        if (mask) {
            const int slot = H + __popcll(mask & below);
            if (in && slot < BQG_HITS) my[slot] = k;
            H += __popcll(mask);
        }
    }
    int n;
    if (H > BQG_HITS) {
        n = wave_ball_query(xyz + (size_t)b * N * 3, N, cx, cy, cz, r2, nsample, lane, out);
    } else {
        pg_wave_sync();
        int first = 0x7fffffff;
        for (int i = lane; i < H; i += 64) {
            const int mine = my[i];
            int r = 0;
            for (int j = 0; j < H; ++j) r += my[j] < mine;
            if (r < nsample) out[r] = mine;
            first = min(first, mine);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
        if (H == 0) first = 0;
        n = H < nsample ? H : nsample;
        for (int s2 = n + lane; s2 < nsample; s2 += 64) out[s2] = first;   // pad with the first hit (0 if none)
    }
    if (lane == 0 && cnt_out) cnt_out[gi] = n;
}

// the operator's shape check, the grid's checks and layout for a cloud of N points, the operator's launch bound: the parent's order
static int bqg_plan(const char* who, int B, int N, int M, int nsample, PointGridPlan* pl) {
    GAD_REQUIRE(B >= 0 && N >= 1 && M >= 0 && nsample >= 1, GAD_ERR_SHAPE, "%s: unsupported shape B=%d N=%d M=%d nsample=%d", who, B, N,
                M, nsample);
    const int rc = point_grid_plan(who, B, N, pl);
    if (rc != GAD_OK) return rc;
    // (hipLaunchKernelGGL takes the grid in threads: B * M / 4 workgroups x 256 has to stay below 2^32)
    GAD_REQUIRE((long long)B * M < (1ll << 26) && B <= 65535, GAD_ERR_SHAPE, "%s: a grid of B * M = %d * %d centroids overflows", who, B, M);
    return GAD_OK;
}

extern "C" long long gad_ball_query_grid_workspace_bytes(int B, int N, int M, int nsample) {
    PointGridPlan pl;
    const int rc = bqg_plan("ball_query_grid_workspace_bytes", B, N, M, nsample, &pl);
    return rc != GAD_OK ? rc : pl.total;
}

extern "C" int gad_ball_query_grid(const float* new_xyz, const float* xyz, int B, int N, int M, float radius, int nsample,
                                   int32_t* idx, int32_t* cnt, void* workspace, void* stream) {
    GAD_REQUIRE(new_xyz && xyz && idx, GAD_ERR_NULL, "ball_query_grid: null pointer (new_xyz / xyz / idx)");
    PointGridPlan pl;
    int rc = bqg_plan("ball_query_grid", B, N, M, nsample, &pl);
    if (rc != GAD_OK) return rc;
    const int G = B * M;
    if (G == 0) return GAD_OK;
    PointGridView v;
    rc = point_grid_carve("ball_query_grid", workspace, pl, &v);
    if (rc != GAD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const float r2 = radius * radius;
    if (!g_geo_opt.bq_grid || !(radius > 0.f && radius < 1.0e18f)) {  // no grid for such a radius: the scan is right for every one
        hipLaunchKernelGGL(ball_query_kernel, dim3(gad_cdiv(G, 4)), dim3(256), 0, st, new_xyz, xyz, G, N, M, r2, nsample, idx, cnt);
        GAD_CHECK_LAUNCH("ball_query_grid(scan)");
        return GAD_OK;
    }
    point_grid_build(xyz, B, N, pl, v, PG_EDGE_RADIUS, radius, nullptr, st);
    hipLaunchKernelGGL(bqg_query_kernel, dim3(gad_cdiv(G, 4)), dim3(256), 0, st, new_xyz, xyz, G, N, M, r2, nsample, pl.cells, v.hdr,
                       v.start, v.sorted, idx, cnt);
    GAD_CHECK_LAUNCH("ball_query_grid");
    return GAD_OK;
}

// QueryAndGroup(use_xyz=True) in one pass: a wavefront owns a centroid, keeps its idx row in LDS,
// then streams the (3+C) grouped channels out as contiguous S-float runs.
__global__ __launch_bounds__(256) void query_and_group_kernel(const float* __restrict__ new_xyz,
                                                              const float* __restrict__ xyz,
                                                              const float* __restrict__ feat, int G, int C,
                                                              int N, int M, float r2, int S,
                                                              int32_t* __restrict__ idx,
                                                              float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) int32_t sidx[];   // 4 waves x S
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + w;
    if (g >= G) return;
    const int b = g / M, m = g - b * M;
    const float* c = new_xyz + (size_t)g * 3;
    const float cx = c[0], cy = c[1], cz = c[2];
    const float* p = xyz + (size_t)b * N * 3;
    int32_t* my = sidx + w * S;
    wave_ball_query(p, N, cx, cy, cz, r2, S, lane, my);
    // LDS writes of this wave are read back by the same wave only
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    int32_t* gi = idx + (size_t)g * S;
    const size_t plane = (size_t)M * S;
    float* o = out + ((size_t)b * (3 + C)) * plane + (size_t)m * S;
    for (int s = lane; s < S; s += 64) {
        const int k = my[s];
        gi[s] = k;
        o[0 * plane + s] = __fsub_rn(p[k * 3 + 0], cx);
        o[1 * plane + s] = __fsub_rn(p[k * 3 + 1], cy);
        o[2 * plane + s] = __fsub_rn(p[k * 3 + 2], cz);
        const float* f = feat + (size_t)b * C * N + k;
        for (int ch = 0; ch < C; ++ch) o[(3 + ch) * plane + s] = f[(size_t)ch * N];
    }
}

extern "C" int gad_query_and_group(const float* new_xyz, const float* xyz, const float* features, int B,
                                   int C, int N, int M, float radius, int nsample, int32_t* idx, float* out,
                                   void* stream) {
    GAD_REQUIRE(new_xyz && xyz && idx && out && (features || C == 0), GAD_ERR_NULL, "query_and_group: null pointer");
    GAD_REQUIRE(nsample >= 1 && nsample <= 4096, GAD_ERR_SHAPE, "query_and_group: nsample out of range");
    const int G = B * M;
    if (G == 0) return GAD_OK;
    static const char* const names[] = {"query_and_group(cells)", "query_and_group(tiled)"};
    const BqRoute r = bq_route(N, nsample, radius);
    if (r != BQ_SCAN) return bq_launch(r, names, new_xyz, xyz, features, B, C, N, M, radius, nsample, idx, nullptr, out, (hipStream_t)stream);
    hipLaunchKernelGGL(query_and_group_kernel, dim3(gad_cdiv(G, 4)), dim3(256), sizeof(int32_t) * 4 * nsample,
                       (hipStream_t)stream, new_xyz, xyz, features, G, C, N, M, radius * radius, nsample, idx,
                       out);
    GAD_CHECK_LAUNCH("query_and_group");
    return GAD_OK;
}
