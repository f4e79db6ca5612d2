// dW pass of the layer-GEMM family (overview and map of the units: gemm.hip): the tile, skinny, streaming, gather-streaming, wide
// and wide-split kernels, dw_reduce_kernel with its launcher, the route predicates and gad_gemm_dw.
#include "gemm_common.hpp"

// ------------------------------------------------------------------------------------------------
// backward wrt the weights:  gacc[n][k] += sum_r dZ[r][n] * X[r][k]
// split over rows: every (tile, split) block writes its partial tile to the caller's workspace, a
// second kernel sums the splits in f64.  Without a workspace: f64 atomics.
// ------------------------------------------------------------------------------------------------
// VM: stride of the per-channel vectors in LDS (>= the widest layer side).  512 instead of VMAX = 1024 brings the
// workgroup from 46 KB to 32 KB of LDS: four instead of three resident workgroups per CU (the register budget allows four).
template <int WM, int WN, int TM, int TN, int XM, bool VEC, int VM>
__global__ __launch_bounds__(256) void gemm_dw_kernel(DzSrc d, XSrc x, Groups gr,
                                                       const int32_t* __restrict__ n_rows_dev, int n_rows_static,
                                                       int Kp, int k_used, int n_ktiles, double* __restrict__ gacc,
                                                       float* __restrict__ partial, long long group_stride, unsigned long long* __restrict__ ts) {
    KTimer kt(ts);
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int PA = PitchD<BM>::v, PB = PitchD<BN>::v;
    constexpr int UA = BM * 8 / 256, UB = BN * 8 / 256;
    constexpr int TILE = KT * PA + KT * PB;
    constexpr int SM = TILE + (VEC ? 5 * VM : 4) + 2 * VM;
    __shared__ __attribute__((aligned(16))) float smem[SM];
    float* As = smem;
    float* Bs = smem + KT * PA;
    float* vec = smem + TILE;
    float* sv = vec + (VEC ? 5 * VM : 4);
    float* tv = sv + VM;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int g = blockIdx.z;
    const int doff = gr.aoff[g], zoff = gr.ooff[g], n_out = gr.nout[g];
    const int tile_n = blockIdx.x / n_ktiles, tile_k = blockIdx.x % n_ktiles;
    const int n0 = tile_n * BM, k0 = tile_k * BN;
    if (n0 >= n_out) return;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    int chunk = gad_cdiv_dev(n_rows, (int)gridDim.y);
    chunk = (chunk + KT - 1) / KT * KT;
    const int r_begin = blockIdx.y * chunk;
    const int r_end = min(r_begin + chunk, n_rows);
    if (r_begin >= r_end) return;     // the reducer skips the same splits (same chunk arithmetic)
    if (VEC) stage_dz_vecs<VM>(vec, d, doff, n_out);
    if (XM == 0 && x.affine) stage_affine<256>(sv, tv, x, zoff, x.c_in);
    __syncthreads();

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[a][b][v] = 0.f;
    DzRaw ra[UA];
    float wa[UA];
    XRaw rb[UB];
    const int bulk = XM == 0 ? x.c_in : x.feat_c;
    const bool tail = k0 + BN > bulk;
    // row -> group / point indices are needed to ADDRESS the pooled-gradient and gather loads: fetched one K-tile
    // ahead of the data they address, so a tile's load phase is one memory latency, not two chained ones
    int gq[UA], pq[UB], xq[UB];
    auto load_idx = [&](int rb0) {
#pragma unroll
        for (int it = 0; it < UA; ++it) {
            int kk, i; unit_D<BM>(it * 256 + tid, kk, i);
            const int r = rb0 + kk;
            gq[it] = d.gmode != 0 ? d.row_grp[r < r_end ? r : 0] : 0;
        }
#pragma unroll
        for (int it = 0; it < UB; ++it) {
            int kk, j; unit_D<BN>(it * 256 + tid, kk, j);
            const int r = rb0 + kk;
            const int rr = r < r_end ? r : 0;
            pq[it] = XM == 1 ? x.row_pt[rr] : 0;
            xq[it] = (XM == 1 && tail) ? x.row_grp[rr] : -1;
        }
    };
    auto load_tile = [&](int rb0) {
#pragma unroll
        for (int it = 0; it < UA; ++it) {
            int kk, i; unit_D<BM>(it * 256 + tid, kk, i);
            const int r = rb0 + kk;
            const bool ok = r < r_end;
            const int rr = ok ? r : 0;
            wa[it] = d.row_w ? d.row_w[rr] : 1.f;
            ra[it] = dz_raw<VEC>(d, r, ok, doff, n0 + i, n_out, gq[it]);
        }
#pragma unroll
        for (int it = 0; it < UB; ++it) {
            int kk, j; unit_D<BN>(it * 256 + tid, kk, j);
            const int r = rb0 + kk;
            const bool ok = r < r_end && (k0 + j < Kp);
            rb[it] = x_raw<XM>(x, r, ok, zoff, k0 + j, tail, pq[it], xq[it]);
        }
        load_idx(rb0 + KT);
    };
    auto store_tile = [&](int rb0) {
#pragma unroll
        for (int it = 0; it < UA; ++it) {
            int kk, i; unit_D<BM>(it * 256 + tid, kk, i);
            const int r = rb0 + kk;
            store_D<BM>(As, kk, i, dz_finish<VEC, VM>(d, ra[it], r, r < r_end, n0 + i, n_out, wa[it], vec));
        }
#pragma unroll
        for (int it = 0; it < UB; ++it) {
            int kk, j; unit_D<BN>(it * 256 + tid, kk, j);
            const int r = rb0 + kk;
            const bool ok = r < r_end && (k0 + j < Kp);
            store_D<BN>(Bs, kk, j, x_finish<XM>(x, rb[it], ok, k0 + j, sv, tv));
        }
    };
    load_idx(r_begin);
    load_tile(r_begin);
    for (int rb0 = r_begin; rb0 < r_end; rb0 += KT) {
        store_tile(rb0);
        __syncthreads();
        if (rb0 + KT < r_end) load_tile(rb0 + KT);
        mfma_ktile<TM, TN, PA, PB>(As, Bs, wm * TM * 32, wn * TN * 32, lane, acc);
        __syncthreads();
    }
    const int l31 = lane & 31, half = lane >> 5;
    float* pout = partial ? partial + (size_t)g * group_stride + (size_t)blockIdx.y * n_out * Kp : nullptr;
    double* aout = gacc + gr.woff[g];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int k = k0 + wn * TN * 32 + tn * 32 + l31;
        if (k >= k_used) continue;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int n = n0 + wm * TM * 32 + tm * 32 + acc_row(v, half);
                if (n >= n_out) continue;
                if (pout) pout[(size_t)n * Kp + k] = acc[tm][tn][v];
                else atomic_add_f64(aout + (size_t)n * Kp + k, (double)acc[tm][tn][v]);
            }
    }
}

#define DW_RED_CHUNK 16
// all_active: every split wrote its partial tile (the streaming kernels deal row units to the splits round-robin); else the
// splits are contiguous row chunks and those past the live rows were not written
__global__ __launch_bounds__(256) void dw_reduce_kernel(const float* __restrict__ partial, long long group_stride,
                                                        Groups gr, const int32_t* __restrict__ n_rows_dev,
                                                        int n_rows_static, int splits, int Kp, int k_used,
                                                        double* __restrict__ gacc, int all_active = 0) {
    const int g = blockIdx.z;
    const int n_out = gr.nout[g];
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)n_out * Kp) return;
    const int k = (int)(e % Kp);
    if (k >= k_used) return;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    int chunk = (n_rows + splits - 1) / splits;
    chunk = (chunk + KT - 1) / KT * KT;
    const int active = all_active ? splits : (chunk > 0 ? (n_rows + chunk - 1) / chunk : 0);
    const int s0 = blockIdx.y * DW_RED_CHUNK, s1 = min(s0 + DW_RED_CHUNK, active);
    if (s0 >= s1) return;
    const float* p = partial + (size_t)g * group_stride + e;
    const size_t stride = (size_t)n_out * Kp;
    double s = 0.0;
#pragma unroll 4
    for (int sidx = s0; sidx < s1; ++sidx) s += (double)p[(size_t)sidx * stride];
    atomic_add_f64(gacc + gr.woff[g] + e, s);
}

int dw_reduce_launch(const float* partial, const Groups& gr, int nmax, const int32_t* n_rows_dev, int rows, int splits, int Kp,
                     int k_used, double* gacc, int all_active, hipStream_t st) {
    hipLaunchKernelGGL(dw_reduce_kernel, dim3(gad_cdiv((long long)nmax * Kp, 256), gad_cdiv(splits, DW_RED_CHUNK), gr.n), dim3(256), 0,
                       st, partial, (long long)splits * nmax * Kp, gr, n_rows_dev, rows, splits, Kp, k_used, gacc, all_active);
    GAD_CHECK_LAUNCH("dw_reduce");
    return GAD_OK;
}

// skinny dW for the small-M layers (FC head, actor / critic heads: <= 1024 rows to reduce over, outputs up to 1024 x 1032).
// One 32x32 tile of dW per workgroup, the 8 wavefronts split the ROWS.  Both MFMA operands are indexed [row][channel]
// in memory with the reduction index (rows) leading, so with the k = 8j+4h+i visiting order lane (channel = lane%32)
// needs four consecutive rows of its channel: four coalesced 4-byte loads each for z, dY (-> dZ in registers, per-lane
// BatchNorm constants) and for the layer input (-> act(scale*z+shift), or the bias / extra column).  No LDS staging,
// all loads of a wavefront's rows in flight before its first MFMA; partial tiles summed through LDS, then f64 atomics
// straight into the gradient arena (no split-K workspace, no reduce launch).
template <int NW>
__global__ __launch_bounds__(64 * NW) void gemm_dw_skinny_kernel(DzSrc d, XSrc x, Groups gr, int n_rows, int Kp,
                                                                    int k_used, double* __restrict__ gacc, unsigned long long* __restrict__ ts) {
    KTimer kt(ts);
    __shared__ float part[NW * 16 * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int g = blockIdx.z;
    const int doff = gr.aoff[g], zoff = gr.ooff[g], n_out = gr.nout[g];
    const int n0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    if (n0 >= n_out) return;
    // A side: this lane's output channel n and its BatchNorm-backward constants
    const int n = n0 + l31;
    const bool n_ok = n < n_out;
    const int ch = doff + (n_ok ? n : 0);
    const float dsc = (d.scale && !d.premasked) ? d.scale[ch] : 1.f, dsh = (d.scale && !d.premasked) ? d.shift[ch] : 0.f;
    float dP, dQ, dS;
    dz_coef(d, ch, dP, dQ, dS);
    // B side: this lane's input column k: 0 = activation column, 1 = extra column, 2 = bias (ones) column, 3 = padding
    const int k = k0 + l31;
    const int kind = k < x.c_in ? 0 : ((k == x.c_in && x.extra) ? 1 : (k == x.ones_col ? 2 : 3));
    const int kc = zoff + (kind == 0 ? k : 0);
    const float xs = (kind == 0 && x.scale) ? x.scale[kc] : 1.f, xt = (kind == 0 && x.shift) ? x.shift[kc] : 0.f;

    const int units = (n_rows + 7) >> 3;
    const int per = (units + NW - 1) / NW;
    const int u0 = wave * per, u1 = min(units, u0 + per);
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    constexpr int CHU = 4;                                   // 8-row units per register chunk
    for (int c0 = u0; c0 < u1; c0 += CHU) {
        float rz[CHU][4], rg[CHU][4], rx[CHU][4], rw[CHU][4];
#pragma unroll
        for (int u = 0; u < CHU; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 8 * (c0 + u) + 4 * half + i;
                const int rr = min(r, max(n_rows - 1, 0));
                rz[u][i] = d.z ? d.z[(size_t)rr * d.z_pitch + ch] : 0.f;
                rg[u][i] = d.G[(size_t)rr * d.g_pitch + ch];
                rw[u][i] = d.row_w ? d.row_w[rr] : 1.f;
                rx[u][i] = kind == 0 ? x.zin[(size_t)rr * x.zin_pitch + kc] : (kind == 1 ? x.extra[rr] : (kind == 2 ? 1.f : 0.f));
            }
#pragma unroll
        for (int u = 0; u < CHU; ++u) {
            if (c0 + u >= u1) break;                         // wave-uniform
            float a4[4], b4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 8 * (c0 + u) + 4 * half + i;
                const bool live = r < n_rows;
                const float z = rz[u][i];
                float gq = rg[u][i];
                if (d.relu && !d.premasked) gq = fmaf(z, dsc, dsh) > 0.f ? gq : 0.f;
                if (d.coef) gq = dP * gq - rw[u][i] * fmaf(dS, z, dQ);
                a4[i] = (live && n_ok) ? gq : 0.f;
                float xv = rx[u][i];
                if (kind == 0) { xv = fmaf(xv, xs, xt); if (x.relu) xv = fmaxf(xv, 0.f); }
                b4[i] = live ? xv : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i], b4[i], acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) part[(wave * 16 + v) * 64 + lane] = acc[v];
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < NW; ++w)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] += part[(w * 16 + v) * 64 + lane];
    if (k >= k_used) return;
    double* aout = gacc + gr.woff[g];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int nn = n0 + acc_row(v, half);
        if (nn < n_out) atomic_add_f64(aout + (size_t)nn * Kp + k, (double)acc[v]);
    }
}

// Streaming dW for the SA1 layers (>= 32k de-duplicated rows, 64 input channels, 64 or 128 output channels).
// dW[n][k] = sum_r dZ[r][n] * X[r][k]: the reduction index is the leading index of both operands in memory, so a lane that
// owns output channel n (A side) / input channel k (B side) feeds the MFMA straight from coalesced 4-byte global loads --
// no LDS tiles, no barriers in the loop, BatchNorm constants per lane in registers (as in the skinny kernel above).
// Work split: a workgroup of 8 wavefronts owns one split of the rows (the dw_reduce geometry: blockIdx.x = split);
// for 128 output channels wavefronts 0-3 take output channels 0-63 and 4-7 take 64-127, each set dealing the split's
// 8-row units among its four members.  Every wavefront keeps a 64 x 64 block of dW in 64 accumulator registers
// (2 x 2 MFMA tiles: each loaded operand is used twice), loads unit u+1 while computing unit u, and the four partial
// blocks are summed through LDS into the split's partial tile.
template <int NG, int GM>
__global__ __launch_bounds__(512) void gemm_dw_stream_kernel(DzSrc d, XSrc x, const int32_t* __restrict__ n_rows_dev,
                                                             int n_rows_static, int splits, float* __restrict__ partial, unsigned long long* __restrict__ ts) {
    KTimer kt(ts);
    constexpr int NO = 64 * NG, KP = 64, RW = 8 / NG;              // RW: wavefronts that share the rows of one column set
    __shared__ float red[8 * 16 * 64];                             // one accumulator tile of every wavefront
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int cset = wave / RW, wr = wave % RW;                    // column set, rank among the wavefronts of that set
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    // 8-row units are dealt to the workgroups ROUND-ROBIN (unit = (k * gridDim.x + blockIdx.x) * RW + rank): at any time
    // the whole grid reads one contiguous window of rows and that window sweeps the arrays front to back -- the order in
    // which the dX kernel of the same layer, running beside this one on the main stream, walks them too, so the second
    // reader of z / dY finds the lines in the L2 / Infinity Cache instead of HBM (contiguous chunks per workgroup touched
    // all of the array at once).  Every workgroup writes its partial tile (zeros without rows): dw_reduce all_active.
    const int r_begin = 0, r_end = n_rows;
    (void)splits;

    // per-lane constants: A side (dZ) output channels n = 64 cset + 32 j + l31, B side (X) input channels k = 32 b + l31
    float dP[2], dQ[2], dS[2], xs[2], xt[2];          // (the ReLU mask is already in dY: premasked)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ch = 64 * cset + 32 * j + l31;
        dz_coef(d, ch, dP[j], dQ[j], dS[j]);
        xs[j] = x.scale[32 * j + l31]; xt[j] = x.shift[32 * j + l31];
    }
    // Addressing of the main loop: raw buffer loads whose per-lane byte offset is a CONSTANT (channel block + the
    // half-wave's 4-row stagger) and whose row position lives in the scalar offset -- no vector ALU work per load.
    const unsigned lane_n = 64u * cset + l31;
    const int zpitch4 = d.z_pitch * 4, xpitch4 = x.zin_pitch * 4, gpitch4 = (GM == 0 ? d.g_pitch : d.c) * 4;
    const __amdgpu_buffer_rsrc_t zr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.z), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t gr_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(GM == 0 ? d.G : d.dout), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(GM == 0 ? d.row_grp : d.argmax), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x.zin), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.row_w ? d.row_w : d.z), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(GM == 0 ? d.argmax : d.row_grp), 0, GAD_BUF_MAX, 0x00020000);
    const int vl_z = 4 * half * zpitch4 + (int)lane_n * 4, vl_x = 4 * half * xpitch4 + l31 * 4;
    const int vl_g = (GM == 0 ? 4 * half * gpitch4 : 0) + (int)lane_n * 4, vl_r = 4 * half * 4;

    struct Unit { float z[4][2], g[4][2], xv[4][2], w[4]; int a[4][2]; };
    auto ldf = [](__amdgpu_buffer_rsrc_t r, int vo, int so) { return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, vo, so, 0)); };
    auto load = [&](Unit& u, int unit) {                           // a unit with all eight rows inside the split
        const int rs = r_begin + 8 * unit;                         // scalar
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            u.w[i] = d.row_w ? ldf(wr_, vl_r, (rs + i) * 4) : 1.f;
            int vg = vl_g;
            if (GM == 1) vg = (int)__builtin_amdgcn_raw_buffer_load_b32(pr, vl_r, (rs + i) * 4, 0) * gpitch4 + vl_g;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                u.z[i][j] = ldf(zr, vl_z + 128 * j, (rs + i) * zpitch4);
                u.g[i][j] = ldf(gr_, vg + 128 * j, GM == 0 ? (rs + i) * gpitch4 : 0);
                if (GM == 1) u.a[i][j] = (int)__builtin_amdgcn_raw_buffer_load_b32(ar, vg + 128 * j, 0, 0);
                u.xv[i][j] = ldf(xr, vl_x + 128 * j, (rs + i) * xpitch4);
            }
        }
    };
    auto load_tail = [&](Unit& u, int unit) {                      // the ragged last unit: clamped rows, plain loads
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = min(r_begin + 8 * unit + 4 * half + i, r_end - 1);
            u.w[i] = d.row_w ? d.row_w[r] : 1.f;
            const size_t go = (GM == 0 ? (size_t)r * d.g_pitch : (size_t)d.row_grp[r] * d.c) + lane_n;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                u.z[i][j] = d.z[(size_t)r * d.z_pitch + lane_n + 32 * j];
                u.g[i][j] = (GM == 0 ? d.G : d.dout)[go + 32 * j];
                if (GM == 1) u.a[i][j] = d.argmax[go + 32 * j];
                u.xv[i][j] = x.zin[(size_t)r * x.zin_pitch + l31 + 32 * j];
            }
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[j][b][v] = 0.f;
    auto compute = [&](const Unit& u, int unit, auto tail) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r_begin + 8 * unit + 4 * half + i;
            const bool live = !decltype(tail)::value || r < r_end;
            float a2[2], b2[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float z = u.z[i][j];
                float gq = u.g[i][j];
                if (GM == 1) gq = u.a[i][j] == r ? gq : 0.f;
                gq = dP[j] * gq - u.w[i] * fmaf(dS[j], z, dQ[j]);
                a2[j] = live ? gq : 0.f;
                const float xv = fmaxf(fmaf(u.xv[i][j], xs[j], xt[j]), 0.f);
                b2[j] = live ? xv : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[j][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[j], b2[b], acc[j][b], 0, 0, 0);
        }
    };
    const std::integral_constant<bool, false> full;
    const std::integral_constant<bool, true> part;
    const int nfull = (r_end - r_begin) >> 3;                      // units with all eight rows live
    const int ustep = gridDim.x * RW;
    Unit u0, u1;
    int un = blockIdx.x * RW + wr;
    if (un < nfull) load(u0, un);
    while (un < nfull) {
        if (un + ustep < nfull) load(u1, un + ustep);
        compute(u0, un, full);
        un += ustep;
        if (un >= nfull) break;
        if (un + ustep < nfull) load(u0, un + ustep);
        compute(u1, un, full);
        un += ustep;
    }
    if (((r_end - r_begin) & 7) != 0 && (nfull / RW) % gridDim.x == blockIdx.x && wr == nfull % RW) {   // the ragged last unit
        load_tail(u0, nfull);
        compute(u0, nfull, part);
    }
    // the set's RW partial 64 x 64 blocks -> one: tile (j, b) of every wavefront through LDS, summed by wavefront (j, b) of the set
    float* pout = partial + (size_t)blockIdx.x * NO * KP;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = t >> 1, b = t & 1;
#pragma unroll
        for (int v = 0; v < 16; ++v) red[(wave * 16 + v) * 64 + lane] = acc[j][b][v];
        __syncthreads();
        if (wr == t % RW) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                float sum = 0.f;
#pragma unroll
                for (int w = 0; w < RW; ++w) sum += red[((cset * RW + w) * 16 + v) * 64 + lane];
                const int n = 64 * cset + 32 * j + acc_row(v, half), k = 32 * b + l31;
                pout[(size_t)n * KP + k] = sum;
            }
        }
        __syncthreads();
    }
}

// Streaming dW for SA1 layer 1, whose input rows are GATHERED: [feat[pt] | src_xyz[pt] - ctr_xyz[grp] | action[sample] | 0]
// (<= 32 columns, no BatchNorm in front).  Same scheme as above with one B tile: lane c of the B side produces input column
// c of its rows from per-lane constants (which array, which stride, which component), the A side is the adjacent-pair
// mapping (accumulator row i of tile j = output channel 2 i + j, one 8-byte load per row for z and for dY).
__global__ __launch_bounds__(512) void gemm_dw_gather_stream_kernel(DzSrc d, XSrc x, const int32_t* __restrict__ n_rows_dev,
                                                                    int n_rows_static, int splits, int Kp, int k_used,
                                                                    float inv_gps, float* __restrict__ partial, unsigned long long* __restrict__ ts) {
    KTimer kt(ts);
    constexpr int RW = 8;
    typedef unsigned gad_u32x2 __attribute__((ext_vector_type(2)));
    __shared__ float red[8 * 16 * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    const int r_begin = 0, r_end = n_rows;         // units dealt round-robin over the grid (see gemm_dw_stream_kernel)
    (void)splits;

    const unsigned lane_n = 2u * l31;
    float dP[2], dQ[2], dS[2];                        // (premasked dY)
#pragma unroll
    for (int j = 0; j < 2; ++j) dz_coef(d, lane_n + j, dP[j], dQ[j], dS[j]);
    // B side: what input column k = l31 is made of
    const int k = l31, fc = x.feat_c;
    const int kind = k < fc ? 0 : (k < fc + 3 ? 1 : ((x.action && k < fc + 3 + x.act_c) ? 2 : 3));
    const float* base1 = kind == 0 ? x.feat : (kind == 1 ? x.src_xyz : (kind == 2 ? x.action : x.feat));
    const int stride1 = kind == 0 ? fc : (kind == 1 ? 3 : (kind == 2 ? x.act_c : 0));
    const int off1 = kind == 0 ? k : (kind == 1 ? k - fc : (kind == 2 ? k - fc - 3 : 0));
    const bool sub_ctr = kind == 1 && x.ctr_xyz != nullptr;
    const float* base2 = sub_ctr ? x.ctr_xyz + off1 : x.src_xyz;   // lanes without a centre read a valid address, unused

    const int zpitch4 = d.z_pitch * 4, gpitch4 = d.g_pitch * 4;
    const __amdgpu_buffer_rsrc_t zr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.z), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t gr_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.G), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.row_w ? d.row_w : d.z), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t ptr_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(x.row_pt), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t grpr = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(x.row_grp), 0, GAD_BUF_MAX, 0x00020000);
    const int vl_z = 4 * half * zpitch4 + (int)lane_n * 4, vl_g = 4 * half * gpitch4 + (int)lane_n * 4, vl_r = 4 * half * 4;

    struct Unit { float z[4][2], g[4][2], w[4], x1[4], x2[4]; };
    auto gather = [&](Unit& u, int i, int pt, int grp) {
        int idx = pt;
        if (kind == 2) {                                           // sample = grp / gps (gps need not be a power of two)
            int q = (int)((float)grp * inv_gps);
            const int rem = grp - q * x.gps;
            q += rem >= x.gps ? 1 : (rem < 0 ? -1 : 0);
            idx = q;
        }
        u.x1[i] = base1[(size_t)idx * stride1 + off1];
        u.x2[i] = base2[sub_ctr ? (size_t)grp * 3 : 0];
    };
    auto load = [&](Unit& u, int unit) {
        const int rs = r_begin + 8 * unit;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int pt = (int)__builtin_amdgcn_raw_buffer_load_b32(ptr_, vl_r, (rs + i) * 4, 0);
            const int grp = (int)__builtin_amdgcn_raw_buffer_load_b32(grpr, vl_r, (rs + i) * 4, 0);
            u.w[i] = d.row_w ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wr_, vl_r, (rs + i) * 4, 0)) : 1.f;
            const gad_u32x2 zz = __builtin_amdgcn_raw_buffer_load_b64(zr, vl_z, (rs + i) * zpitch4, 0);
            const gad_u32x2 gg = __builtin_amdgcn_raw_buffer_load_b64(gr_, vl_g, (rs + i) * gpitch4, 0);
            u.z[i][0] = __uint_as_float(zz.x); u.z[i][1] = __uint_as_float(zz.y);
            u.g[i][0] = __uint_as_float(gg.x); u.g[i][1] = __uint_as_float(gg.y);
            gather(u, i, pt, grp);
        }
    };
    auto load_tail = [&](Unit& u, int unit) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = min(r_begin + 8 * unit + 4 * half + i, r_end - 1);
            u.w[i] = d.row_w ? d.row_w[r] : 1.f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                u.z[i][j] = d.z[(size_t)r * d.z_pitch + lane_n + j];
                u.g[i][j] = d.G[(size_t)r * d.g_pitch + lane_n + j];
            }
            gather(u, i, x.row_pt[r], x.row_grp[r]);
        }
    };
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[j][v] = 0.f;
    auto compute = [&](const Unit& u, int unit, auto tail) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r_begin + 8 * unit + 4 * half + i;
            const bool live = !decltype(tail)::value || r < r_end;
            float xv = sub_ctr ? __fsub_rn(u.x1[i], u.x2[i]) : u.x1[i];
            xv = (kind != 3 && live) ? xv : 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float z = u.z[i][j];
                const float gq = dP[j] * u.g[i][j] - u.w[i] * fmaf(dS[j], z, dQ[j]);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(live ? gq : 0.f, xv, acc[j], 0, 0, 0);
            }
        }
    };
    const std::integral_constant<bool, false> full;
    const std::integral_constant<bool, true> part;
    const int nfull = (r_end - r_begin) >> 3;
    const int ustep = gridDim.x * RW;
    Unit u0, u1;
    int un = blockIdx.x * RW + wave;
    if (un < nfull) load(u0, un);
    while (un < nfull) {
        if (un + ustep < nfull) load(u1, un + ustep);
        compute(u0, un, full);
        un += ustep;
        if (un >= nfull) break;
        if (un + ustep < nfull) load(u0, un + ustep);
        compute(u1, un, full);
        un += ustep;
    }
    if (((r_end - r_begin) & 7) != 0 && (nfull / RW) % gridDim.x == blockIdx.x && wave == nfull % RW) {
        load_tail(u0, nfull);
        compute(u0, nfull, part);
    }
    float* pout = partial + (size_t)blockIdx.x * 64 * Kp;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int v = 0; v < 16; ++v) red[(wave * 16 + v) * 64 + lane] = acc[j][v];
        __syncthreads();
        if ((wave >> 2) == j) {                                    // four wavefronts per tile, four accumulator rows each
#pragma unroll
            for (int vv = 0; vv < 4; ++vv) {
                const int v = 4 * (wave & 3) + vv;
                float sum = 0.f;
#pragma unroll
                for (int w = 0; w < RW; ++w) sum += red[(w * 16 + v) * 64 + lane];
                const int n = 2 * acc_row(v, half) + j;
                if (l31 < Kp) pout[(size_t)n * Kp + l31] = l31 < k_used ? sum : 0.f;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// wide-tile dW for the MID-SIZE layers: dW[n][k] = sum_r dZ[r][n] * X[r][k] is a tiny output (128 x 128 ... 512 x 256)
// behind a long reduction (8e3 - 3e4 rows).  The 64 x 64 kernel re-reads every row of dZ and X once per output tile (4 - 32
// times through L2: 112 MB of traffic for 42 MB of operands) and keeps one accumulator per wavefront.  Here a workgroup owns
// a 128 x 128 block of dW for its chunk of rows -- the whole matrix for the 128-wide layers -- a wavefront 64 x 64 (four
// accumulators: each staged operand value feeds two MFMAs), K-tile = 32 rows, LDS double-buffered with one barrier per
// K-tile, operands stored as loaded ([row][128 + 4]: one ds_write_b128 per staged float4, fragments are conflict-free
// ds_read_b32 of consecutive channels).  dZ = P*dY - w*(Q + S*z) and X = relu(scale*z_in + shift) are formed once per
// staged element.  Partial tiles go to the caller's workspace, dw_reduce sums the row chunks in f64.
// XM = 1 (first layer of SA2 / SA3: gathered input [feat[pt] | src_xyz[pt] - ctr_xyz[grp]]): the X side is feat[pt] as
// stored (row -> point indices fetched one K-tile ahead of the rows they address); the three coordinate columns of dW are
// sums of dZ * dx accumulated with vector FMAs while dZ is staged (12 per float4) by the workgroups of the first k block.
// ------------------------------------------------------------------------------------------------
template <int XM, int GM>
__global__ __launch_bounds__(256, 2) void gemm_dw_wide_kernel(DzSrc d, XSrc x, const int32_t* __restrict__ n_rows_dev,
                                                              int n_rows_static, int Kp, int n_out, int tiles_k,
                                                              float* __restrict__ partial, unsigned long long* __restrict__ ts) {
    KTimer kt_(ts);
    constexpr int BT = 128, P = BT + 4, STAGE = 2 * KT * P, VM = 512;
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE + 5 * VM];
    float* vP = smem + 2 * STAGE;                        // P | Q | S of the dZ channels, scale | shift of the input channels
    float* sv = vP + 3 * VM;
    float* tv = sv + VM;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, half = lane >> 5;
    const int n0 = (blockIdx.x / tiles_k) * BT, k0 = (blockIdx.x % tiles_k) * BT;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    int chunk = gad_cdiv_dev(n_rows, (int)gridDim.y);
    chunk = (chunk + KT - 1) / KT * KT;                  // == dw_reduce_kernel's split geometry
    const int r_begin = blockIdx.y * chunk, r_end = min(r_begin + chunk, n_rows);
    if (r_begin >= r_end) return;                        // the reducer skips the same splits
    for (int i = tid; i < BT; i += 256) {
        float Pc, Qc, Sc;
        dz_coef(d, n0 + i, Pc, Qc, Sc, blockIdx.y == 0 && k0 == 0);
        vP[i] = Pc; vP[VM + i] = Qc; vP[2 * VM + i] = Sc;
        if (XM == 0) { sv[i] = x.scale[k0 + i]; tv[i] = x.shift[k0 + i]; }
    }
    const bool coords = XM == 1 && k0 == 0;              // this workgroup also forms dW[n][feat_c .. feat_c + 2]
    float wx[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) { wx[j][0] = 0.f; wx[j][1] = 0.f; wx[j][2] = 0.f; }
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[a][b][v] = 0.f;
    // staging: a K-tile is 32 rows x 128 channels per side = 1024 float4: thread -> rows sr + 8 u (u < 4), channels c4 .. c4 + 3
    const int c4 = (tid & 31) * 4, sr = tid >> 5;
    const int gpitch = GM == 0 ? d.g_pitch : d.c;
    float4 rz[4], rg[4], rx[4];
    int4 ra[4];
    float rw[4], rd[4][3];
    int pq[4], gq[4];                                    // XM = 1: point / group of the NEXT tile's rows
    int gd[4];                                           // GM = 1: group of the NEXT tile's rows (pooled gradient source)
    auto load_idx = [&](int rb0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = rb0 + sr + 8 * u;
            const int rr = r < r_end ? r : r_end - 1;
            pq[u] = XM == 1 ? x.row_pt[rr] : 0;
            gq[u] = (XM == 1 && x.ctr_xyz) ? x.row_grp[rr] : 0;
            gd[u] = GM == 1 ? d.row_grp[rr] : 0;
        }
    };
    auto load_regs = [&](int rb0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = rb0 + sr + 8 * u;
            const int rr = r < r_end ? r : r_end - 1;
            rw[u] = d.row_w ? d.row_w[rr] : 1.f;
            rz[u] = ldg4(d.z + (size_t)rr * d.z_pitch + n0 + c4);
            if (GM == 0) {
                rg[u] = ldg4(d.G + (size_t)rr * gpitch + n0 + c4);
            } else {
                const int grp = gd[u];                   // (fetched one K-tile ahead: one memory round trip here, not two)
                ra[u] = *reinterpret_cast<const int4*>(d.argmax + (size_t)grp * gpitch + n0 + c4);
                rg[u] = ldg4(d.dout + (size_t)grp * gpitch + n0 + c4);
            }
            if (XM == 0) {
                rx[u] = ldg4(x.zin + (size_t)rr * x.zin_pitch + k0 + c4);
            } else {
                rx[u] = ldg4(x.feat + (size_t)pq[u] * x.feat_c + k0 + c4);
                if (coords) {
                    const float* p = x.src_xyz + (size_t)pq[u] * 3;
                    float q0 = p[0], q1 = p[1], q2 = p[2];
                    if (x.ctr_xyz) {
                        const float* cp = x.ctr_xyz + (size_t)gq[u] * 3;
                        q0 = __fsub_rn(q0, cp[0]); q1 = __fsub_rn(q1, cp[1]); q2 = __fsub_rn(q2, cp[2]);
                    }
                    rd[u][0] = q0; rd[u][1] = q1; rd[u][2] = q2;
                }
            }
        }
        if (XM == 1 || GM == 1) load_idx(rb0 + KT);
    };
    auto write_lds = [&](int it, int rb0) {
        float* As = smem + (it & 1) * STAGE;
        float* Bs = As + KT * P;
        const float4 Pv = *reinterpret_cast<const float4*>(vP + c4), Qv = *reinterpret_cast<const float4*>(vP + VM + c4);
        const float4 Sv = *reinterpret_cast<const float4*>(vP + 2 * VM + c4);
        float4 s4 = f4zero(), t4 = f4zero();
        if (XM == 0) { s4 = *reinterpret_cast<const float4*>(sv + c4); t4 = *reinterpret_cast<const float4*>(tv + c4); }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = rb0 + sr + 8 * u;
            float4 g = rg[u];
            const float4 z = rz[u];
            if (GM == 1) {
                g.x = ra[u].x == r ? g.x : 0.f; g.y = ra[u].y == r ? g.y : 0.f;
                g.z = ra[u].z == r ? g.z : 0.f; g.w = ra[u].w == r ? g.w : 0.f;
            }
            const float w = rw[u];
            float4 a, b;
            a.x = Pv.x * g.x - w * fmaf(Sv.x, z.x, Qv.x); a.y = Pv.y * g.y - w * fmaf(Sv.y, z.y, Qv.y);
            a.z = Pv.z * g.z - w * fmaf(Sv.z, z.z, Qv.z); a.w = Pv.w * g.w - w * fmaf(Sv.w, z.w, Qv.w);
            if (XM == 0) {
                b.x = fmaxf(fmaf(rx[u].x, s4.x, t4.x), 0.f); b.y = fmaxf(fmaf(rx[u].y, s4.y, t4.y), 0.f);
                b.z = fmaxf(fmaf(rx[u].z, s4.z, t4.z), 0.f); b.w = fmaxf(fmaf(rx[u].w, s4.w, t4.w), 0.f);
            } else {
                b = rx[u];
            }
            if (r >= r_end) { a = f4zero(); b = f4zero(); }
            if (coords) {
#pragma unroll
                for (int dd = 0; dd < 3; ++dd) {
                    wx[0][dd] = fmaf(a.x, rd[u][dd], wx[0][dd]); wx[1][dd] = fmaf(a.y, rd[u][dd], wx[1][dd]);
                    wx[2][dd] = fmaf(a.z, rd[u][dd], wx[2][dd]); wx[3][dd] = fmaf(a.w, rd[u][dd], wx[3][dd]);
                }
            }
            *reinterpret_cast<float4*>(As + (sr + 8 * u) * P + c4) = a;
            *reinterpret_cast<float4*>(Bs + (sr + 8 * u) * P + c4) = b;
        }
    };
    if (XM == 1 || GM == 1) load_idx(r_begin);
    load_regs(r_begin);
    __syncthreads();                                     // vP / sv / tv visible
    write_lds(0, r_begin);
    if (r_begin + KT < r_end) load_regs(r_begin + KT);
    __syncthreads();
    int it = 0;
    for (int rb0 = r_begin; rb0 < r_end; rb0 += KT, ++it) {
        const float* As = smem + (it & 1) * STAGE + half * P + wm * 64 + l31;
        const float* Bs = smem + (it & 1) * STAGE + KT * P + half * P + wn * 64 + l31;
#pragma unroll
        for (int s = 0; s < KT / 2; ++s) {
            const float a0 = As[2 * s * P], a1 = As[2 * s * P + 32];
            const float b0 = Bs[2 * s * P], b1 = Bs[2 * s * P + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (rb0 + KT < r_end) write_lds(it + 1, rb0 + KT);
        if (rb0 + 2 * KT < r_end) load_regs(rb0 + 2 * KT);
        __syncthreads();
    }
    float* pout = partial + (size_t)blockIdx.y * n_out * Kp;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int n = n0 + wm * 64 + a * 32 + acc_row(v, half), k = k0 + wn * 64 + b * 32 + l31;
                pout[(size_t)n * Kp + k] = acc[a][b][v];
            }
    if (coords) {                                        // eight staging rows per channel quad -> one sum (the tile LDS is free)
        float* red = smem;                               // [8][128][3]
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int dd = 0; dd < 3; ++dd) red[(sr * BT + c4 + j) * 3 + dd] = wx[j][dd];
        __syncthreads();
        for (int i = tid; i < BT * 3; i += 256) {
            float sum = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) sum += red[q * BT * 3 + i];
            pout[(size_t)(n0 + i / 3) * Kp + x.feat_c + i % 3] = sum;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// wide-tile dW in split-bf16 form (option "mfma_split", GAD_SPLIT_DW_WIDE): the same 128 x 128 block per workgroup, 64 x 64
// per wavefront, K-tile = 32 rows.  The reduction index (rows) is the SLOW index of both operands in memory, while
// v_mfma_f32_32x32x16_bf16 wants 8 consecutive reduction indices per lane: so a thread stages a 4-row x 4-channel patch
// (rows 4 rq .. + 3 of the K-tile, channels 4 cq .. + 3; rq = tid & 7: a wavefront's loads cover 8 rows x 128 contiguous
// bytes), forms dZ / the activated input in registers, splits ROW PAIRS of one channel into hi / mid / lo and stores
// 8 bytes (four rows) per channel and plane into LDS laid out [plane][channel][32 rows] (64-byte rows, 16-byte chunks
// XOR-swizzled by (channel >> 2) & 3: fragments are conflict-free ds_read_b128 of 8 consecutive rows).  Rows 16 .. 31 of every
// K-tile carry NEGATED dZ and accumulate into the second accumulator set (the bf16 MFMA's truncation bias cancels in the
// difference).  One workgroup per CU (eight accumulators per wavefront), LDS double-buffered, one barrier per K-tile.
// ------------------------------------------------------------------------------------------------
template <int XM, int GM>
__global__ __launch_bounds__(256, 1) void gemm_dw_wide_split_kernel(DzSrc d, XSrc x, const int32_t* __restrict__ n_rows_dev,
                                                                    int n_rows_static, int Kp, int n_out, int tiles_k,
                                                                    float* __restrict__ partial, unsigned long long* __restrict__ ts) {
    KTimer kt_(ts);
    constexpr int BT = 128, OPL = BT * 64, STAGE = 6 * OPL, VM = 512;      // bytes: one operand plane, one stage (A planes | B planes)
    __shared__ __attribute__((aligned(16))) unsigned char smem_b[2 * STAGE];
    __shared__ __attribute__((aligned(16))) float vP[5 * VM];               // P | Q | S of the dZ channels, scale | shift of the input channels
    float* sv = vP + 3 * VM;
    float* tv = sv + VM;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, half = lane >> 5;
    const int n0 = (blockIdx.x / tiles_k) * BT, k0 = (blockIdx.x % tiles_k) * BT;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    int chunk = gad_cdiv_dev(n_rows, (int)gridDim.y);
    chunk = (chunk + KT - 1) / KT * KT;                  // == dw_reduce_kernel's split geometry
    const int r_begin = blockIdx.y * chunk, r_end = min(r_begin + chunk, n_rows);
    if (r_begin >= r_end) return;                        // the reducer skips the same splits
    for (int i = tid; i < BT; i += 256) {
        float Pc, Qc, Sc;
        dz_coef(d, n0 + i, Pc, Qc, Sc, blockIdx.y == 0 && k0 == 0);
        vP[i] = Pc; vP[VM + i] = Qc; vP[2 * VM + i] = Sc;
        if (XM == 0) { sv[i] = x.scale[k0 + i]; tv[i] = x.shift[k0 + i]; }
    }
    const bool coords = XM == 1 && k0 == 0;              // this workgroup also forms dW[n][feat_c .. feat_c + 2]
    float wx[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) { wx[j][0] = 0.f; wx[j][1] = 0.f; wx[j][2] = 0.f; }
    f32x16 acc[2][2], an[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) { acc[a][b][v] = 0.f; an[a][b][v] = 0.f; }
    // staging patch of this thread: rows 4 rq + u (u < 4) of the K-tile, channels c4 .. c4 + 3
    const int rq = tid & 7, c4 = (tid >> 3) * 4;
    const float sgn = rq >= 4 ? -1.f : 1.f;              // rows 16 .. 31: negated dZ
    const int gpitch = GM == 0 ? d.g_pitch : d.c;
    float4 rz[4], rg[4], rx[4];
    int4 ra[4];
    float rw[4], rd[4][3];
    int pq[4], gq[4], gd[4];                             // point / group of the NEXT tile's rows (gathered input, pooled gradient)
    auto load_idx = [&](int rb0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = rb0 + 4 * rq + u;
            const int rr = r < r_end ? r : r_end - 1;
            pq[u] = XM == 1 ? x.row_pt[rr] : 0;
            gq[u] = (XM == 1 && x.ctr_xyz) ? x.row_grp[rr] : 0;
            gd[u] = GM == 1 ? d.row_grp[rr] : 0;
        }
    };
    auto load_regs = [&](int rb0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = rb0 + 4 * rq + u;
            const int rr = r < r_end ? r : r_end - 1;
            rw[u] = d.row_w ? d.row_w[rr] : 1.f;
            rz[u] = ldg4(d.z + (size_t)rr * d.z_pitch + n0 + c4);
            if (GM == 0) {
                rg[u] = ldg4(d.G + (size_t)rr * gpitch + n0 + c4);
            } else {
                const int grp = gd[u];
                ra[u] = *reinterpret_cast<const int4*>(d.argmax + (size_t)grp * gpitch + n0 + c4);
                rg[u] = ldg4(d.dout + (size_t)grp * gpitch + n0 + c4);
            }
            if (XM == 0) {
                rx[u] = ldg4(x.zin + (size_t)rr * x.zin_pitch + k0 + c4);
            } else {
                rx[u] = ldg4(x.feat + (size_t)pq[u] * x.feat_c + k0 + c4);
                if (coords) {
                    const float* p = x.src_xyz + (size_t)pq[u] * 3;
                    float q0 = p[0], q1 = p[1], q2 = p[2];
                    if (x.ctr_xyz) {
                        const float* cp = x.ctr_xyz + (size_t)gq[u] * 3;
                        q0 = __fsub_rn(q0, cp[0]); q1 = __fsub_rn(q1, cp[1]); q2 = __fsub_rn(q2, cp[2]);
                    }
                    rd[u][0] = q0; rd[u][1] = q1; rd[u][2] = q2;
                }
            }
        }
        if (XM == 1 || GM == 1) load_idx(rb0 + KT);
    };
    // [plane][channel][rows]: this thread's 8 bytes (rows 4 rq .. + 3) of channel c4 + j
    const int wr_off = c4 * 64 + (rq & 1) * 8, wr_q = rq >> 1;
    auto write_lds = [&](int it, int rb0) {
        unsigned char* As = smem_b + (it & 1) * STAGE;
        unsigned char* Bs = As + 3 * OPL;
        const float4 Pv = *reinterpret_cast<const float4*>(vP + c4), Qv = *reinterpret_cast<const float4*>(vP + VM + c4);
        const float4 Sv = *reinterpret_cast<const float4*>(vP + 2 * VM + c4);
        float4 s4 = f4zero(), t4 = f4zero();
        if (XM == 0) { s4 = *reinterpret_cast<const float4*>(sv + c4); t4 = *reinterpret_cast<const float4*>(tv + c4); }
        float av[4][4], bv[4][4];                        // [row u][channel j]
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = rb0 + 4 * rq + u;
            float4 g = rg[u];
            const float4 z = rz[u];
            if (GM == 1) {
                g.x = ra[u].x == r ? g.x : 0.f; g.y = ra[u].y == r ? g.y : 0.f;
                g.z = ra[u].z == r ? g.z : 0.f; g.w = ra[u].w == r ? g.w : 0.f;
            }
            const float w = rw[u];
            float4 a, b;
            a.x = Pv.x * g.x - w * fmaf(Sv.x, z.x, Qv.x); a.y = Pv.y * g.y - w * fmaf(Sv.y, z.y, Qv.y);
            a.z = Pv.z * g.z - w * fmaf(Sv.z, z.z, Qv.z); a.w = Pv.w * g.w - w * fmaf(Sv.w, z.w, Qv.w);
            if (XM == 0) {
                b.x = fmaxf(fmaf(rx[u].x, s4.x, t4.x), 0.f); b.y = fmaxf(fmaf(rx[u].y, s4.y, t4.y), 0.f);
                b.z = fmaxf(fmaf(rx[u].z, s4.z, t4.z), 0.f); b.w = fmaxf(fmaf(rx[u].w, s4.w, t4.w), 0.f);
            } else {
                b = rx[u];
            }
            if (r >= r_end) { a = f4zero(); b = f4zero(); }
            if (coords) {
#pragma unroll
                for (int dd = 0; dd < 3; ++dd) {
                    wx[0][dd] = fmaf(a.x, rd[u][dd], wx[0][dd]); wx[1][dd] = fmaf(a.y, rd[u][dd], wx[1][dd]);
                    wx[2][dd] = fmaf(a.z, rd[u][dd], wx[2][dd]); wx[3][dd] = fmaf(a.w, rd[u][dd], wx[3][dd]);
                }
            }
            av[u][0] = a.x * sgn; av[u][1] = a.y * sgn; av[u][2] = a.z * sgn; av[u][3] = a.w * sgn;
            bv[u][0] = b.x; bv[u][1] = b.y; bv[u][2] = b.z; bv[u][3] = b.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int off = wr_off + j * 64 + (((wr_q ^ (((c4 + j) >> 2) & 3))) << 4);
            unsigned h0, m0, l0, h1, m1, l1;
            gad_split2(av[0][j], av[1][j], h0, m0, l0);
            gad_split2(av[2][j], av[3][j], h1, m1, l1);
            *reinterpret_cast<uint2*>(As + off) = make_uint2(h0, h1);
            *reinterpret_cast<uint2*>(As + OPL + off) = make_uint2(m0, m1);
            *reinterpret_cast<uint2*>(As + 2 * OPL + off) = make_uint2(l0, l1);
            gad_split2(bv[0][j], bv[1][j], h0, m0, l0);
            gad_split2(bv[2][j], bv[3][j], h1, m1, l1);
            *reinterpret_cast<uint2*>(Bs + off) = make_uint2(h0, h1);
            *reinterpret_cast<uint2*>(Bs + OPL + off) = make_uint2(m0, m1);
            *reinterpret_cast<uint2*>(Bs + 2 * OPL + off) = make_uint2(l0, l1);
        }
    };
    if (XM == 1 || GM == 1) load_idx(r_begin);
    load_regs(r_begin);
    __syncthreads();                                     // vP / sv / tv visible
    write_lds(0, r_begin);
    if (r_begin + KT < r_end) load_regs(r_begin + KT);
    __syncthreads();
    // fragment addressing: channel rows wm * 64 + a * 32 + l31 (A) / wn * 64 + b * 32 + l31 (B); chunk 2 st + half, swizzled
    const int fo = ((half ^ ((l31 >> 2) & 3)) << 4);
    const int arow = (wm * 64 + l31) * 64, brow = 3 * OPL + (wn * 64 + l31) * 64;
    int it = 0;
    for (int rb0 = r_begin; rb0 < r_end; rb0 += KT, ++it) {
        const unsigned char* st = smem_b + (it & 1) * STAGE;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const int off = fo ^ (s2 << 5);
            gad_u32x4 A[2][3], B[2][3];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    A[a][pl] = *reinterpret_cast<const gad_u32x4*>(st + arow + a * (32 * 64) + pl * OPL + off);
                    B[a][pl] = *reinterpret_cast<const gad_u32x4*>(st + brow + a * (32 * 64) + pl * OPL + off);
                }
            // the six products of weight >= 2^-16, smallest first: (A plane, B plane) = (lo, hi) (hi, lo) (mid, mid) (mid, hi) (hi, mid) (hi, hi)
#define GAD_SPD(PA, PB_)                                                                                                       \
            _Pragma("unroll") for (int a = 0; a < 2; ++a) _Pragma("unroll") for (int b = 0; b < 2; ++b) {                      \
                if (s2) an[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gad_as_bf16x8(A[a][PA]), gad_as_bf16x8(B[b][PB_]), an[a][b], 0, 0, 0); \
                else acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gad_as_bf16x8(A[a][PA]), gad_as_bf16x8(B[b][PB_]), acc[a][b], 0, 0, 0); \
            }
            GAD_SPD(2, 0) GAD_SPD(0, 2) GAD_SPD(1, 1) GAD_SPD(1, 0) GAD_SPD(0, 1) GAD_SPD(0, 0)
#undef GAD_SPD
        }
        if (rb0 + KT < r_end) write_lds(it + 1, rb0 + KT);
        if (rb0 + 2 * KT < r_end) load_regs(rb0 + 2 * KT);
        __syncthreads();
    }
    float* pout = partial + (size_t)blockIdx.y * n_out * Kp;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int n = n0 + wm * 64 + a * 32 + acc_row(v, half), k = k0 + wn * 64 + b * 32 + l31;
                pout[(size_t)n * Kp + k] = acc[a][b][v] - an[a][b][v];
            }
    if (coords) {                                        // 8 row quads per channel quad -> one sum (the tile LDS is free)
        float* red = reinterpret_cast<float*>(smem_b);   // [8][128][3]
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int dd = 0; dd < 3; ++dd) red[(rq * BT + c4 + j) * 3 + dd] = wx[j][dd];
        __syncthreads();
        for (int i = tid; i < BT * 3; i += 256) {
            float sum = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) sum += red[q * BT * 3 + i];
            pout[(size_t)(n0 + i / 3) * Kp + x.feat_c + i % 3] = sum;
        }
    }
}

// the wide-tile dW covers: ACT input with BatchNorm + ReLU in front, one group, 128-multiples on both sides, no bias / extra column
static bool dw_wideable(const gad_gemm_dw_args& a, int k_used, bool vec) {
    const gad_gemm_fwd_args& in = a.in;
    const gad_dz_src& d = a.dz;
    if (g_opt.deterministic || !g_opt.dw_wide || !vec || in.n_groups != 1 || in.zin_off[0] != 0 || a.dz_off[0] != 0) return false;
    if (in.n_rows < 2048 || in.n_out[0] % 128 != 0 || in.n_out[0] > 512 || in.ones_col >= 0) return false;
    if (in.mode == 1) {                                  // gathered first layer: features a multiple of 128, + 3 coordinates
        if (g_opt.dw_wide == 2 || d.gmode != 0 || in.act_c != 0 || in.feat_c % 128 != 0 || in.feat_c > 512) return false;
        if (in.Kp != ((in.feat_c + 3 + 7) & ~7) || k_used != in.feat_c + 3) return false;
    } else {
        if (in.Kp % 128 != 0 || in.Kp > 512 || k_used != in.Kp) return false;
        if (in.c_in != in.Kp || !in.scale || !in.shift || !in.relu || in.extra) return false;
    }
    if (!d.z || d.z_pitch % 4 != 0 || !d.relu || !d.premasked || !(d.coefP && d.coefQ && d.coefS)) return false;
    if (d.gmode == 0 ? (d.g_pitch % 4 != 0 || !d.G) : (d.c % 4 != 0)) return false;
    return a.partial != nullptr && a.row_splits <= 0;
}

static bool dw_gather_streamable(const gad_gemm_dw_args& a, int k_used) {
    const gad_gemm_fwd_args& in = a.in;
    const gad_dz_src& d = a.dz;
    if (g_opt.deterministic || !g_opt.dw_stream || in.mode != 1 || in.n_groups != 1 || in.Kp > 32 || in.n_out[0] != 64 || k_used > in.Kp) return false;
    if (in.zin_off[0] != 0 || a.dz_off[0] != 0 || in.n_rows < 32768 || d.gmode != 0 || !d.G) return false;
    if (!d.z || !d.scale || !d.relu || !d.premasked || !(d.coefP && d.coefQ && d.coefS)) return false;
    if (in.feat_c + 3 + (in.action ? in.act_c : 0) > in.Kp) return false;
    if (!a.partial || 256ll * 64 * in.Kp > a.partial_elems) return false;
    return a.row_splits <= 0;
}

bool dw_streamable(const gad_gemm_dw_args& a, int k_used) {
    const gad_gemm_fwd_args& in = a.in;
    const gad_dz_src& d = a.dz;
    if (g_opt.deterministic || !g_opt.dw_stream || in.mode != 0 || in.n_groups != 1 || in.Kp != 64 || in.c_in != 64 || k_used != 64) return false;
    if (in.zin_off[0] != 0 || a.dz_off[0] != 0 || (in.n_out[0] != 64 && in.n_out[0] != 128)) return false;   // w_off: arena offset, dw_reduce applies it
    if (in.n_rows < 32768 || !in.scale || !in.shift || !in.relu || in.extra || in.ones_col >= 0) return false;
    if (!d.z || !d.scale || !d.relu || !d.premasked || !(d.coefP && d.coefQ && d.coefS)) return false;
    if (d.gmode != 0 && d.c != in.n_out[0]) return false;
    if (!a.partial || (long long)DW_STREAM_SPLITS * in.n_out[0] * 64 > a.partial_elems) return false;
    return a.row_splits <= 0;
}

// deterministic mode: the zeroed partial-dW slab of a split generic dW launch (splits past the live rows write nothing: zeros)
static float* det_dw_slab(long long elems, void* stream) {
    float* p = static_cast<float*>(gad_det_scratch(stream, GAD_DET_SLOTS2, (size_t)elems * sizeof(float)));
    if (p && hipMemsetAsync(p, 0, (size_t)elems * sizeof(float), (hipStream_t)stream) != hipSuccess) {
        gad_set_error("deterministic mode: clearing the partial dW slab failed");
        return nullptr;
    }
    return p;
}

extern "C" int gad_gemm_dw(const gad_gemm_dw_args* a, void* stream) {
    unsigned long long* ts = gad_take_timing_slot(stream);
    GAD_REQUIRE(a && a->gacc, GAD_ERR_NULL, "gemm_dw: null pointer");
    const gad_gemm_fwd_args& in = a->in;
    GAD_REQUIRE(in.n_groups >= 1 && in.n_groups <= GAD_MAX_GROUPS, GAD_ERR_SHAPE, "gemm_dw: n_groups");
    GAD_REQUIRE(in.Kp % 8 == 0, GAD_ERR_SHAPE, "gemm_dw: Kp must be a multiple of 8");
    if (int e = check_input(in, "gemm_dw")) return e;
    GAD_REQUIRE(a->dz.gmode == 0 ? a->dz.G != nullptr : (a->dz.argmax && a->dz.dout && a->dz.row_grp), GAD_ERR_NULL,
                "gemm_dw: gradient source");
    if (in.n_rows <= 0) return GAD_OK;
    XSrc x = make_xsrc(in);
    DzSrc d = make_dzsrc(a->dz);
    // group g: dz channel offset dz_off[g], input channel offset zin_off[g], weights at w_off[g]
    Groups gr = make_groups(in.n_groups, a->dz_off, in.w_off, in.zin_off, in.n_out);
    const int nmax = max_nout(gr);
    int k_used = in.mode == 0 ? in.c_in + (in.extra ? 1 : 0) : in.feat_c + 3 + in.act_c;
    if (in.ones_col >= k_used) k_used = in.ones_col + 1;
    if (k_used > in.Kp) k_used = in.Kp;
    hipStream_t st = (hipStream_t)stream;
    const int rows = in.n_rows;
    const bool vec = dz_vectorizable(a->dz, a->dz_off, in.n_out, in.n_groups);
    const bool skinny_route = !g_opt.deterministic && g_opt.dw_skinny && in.mode == 0 && a->dz.gmode == 0 && !in.n_rows_dev && rows <= 1024;
    if (a->dz.bn_dbeta && (skinny_route || dw_gather_streamable(*a, k_used) || dw_streamable(*a, k_used))) {
        gad_dz_src dz2 = a->dz;                          // these kernels read P / Q / S per lane: gad_bn_bwd_coef first
        if (int e2 = coef_fallback(dz2, stream)) return e2;
        d = make_dzsrc(dz2);
    }
    if (skinny_route) {
        GAD_LAUNCH_SKINNY(gemm_dw_skinny_kernel, dim3(gad_cdiv(nmax, 32), gad_cdiv(k_used, 32), gr.n), st, d, x, gr, rows, in.Kp, k_used,
                          a->gacc, ts);
        GAD_CHECK_LAUNCH("gemm_dw(skinny)");
        return GAD_OK;
    }
    if (dw_gather_streamable(*a, k_used)) {
        const int splits = 256;
        const int gps = in.grp_per_sample > 0 ? in.grp_per_sample : 1;
        hipLaunchKernelGGL(gemm_dw_gather_stream_kernel, dim3(splits), dim3(512), 0, st, d, x, in.n_rows_dev, rows, splits, in.Kp, k_used,
                           1.0f / (float)gps, a->partial, ts);
        GAD_CHECK_LAUNCH("gemm_dw(gather stream)");
        return dw_reduce_launch(a->partial, gr, nmax, in.n_rows_dev, rows, splits, in.Kp, k_used, a->gacc, 1, st);
    }
    if (dw_streamable(*a, k_used)) {
        const int splits = DW_STREAM_SPLITS;
        float* part = a->partial;
        if (in.n_out[0] == 64) {
            if (a->dz.gmode == 0) hipLaunchKernelGGL((gemm_dw_stream_kernel<1, 0>), dim3(splits), dim3(512), 0, st, d, x, in.n_rows_dev, rows, splits, part, ts);
            else                  hipLaunchKernelGGL((gemm_dw_stream_kernel<1, 1>), dim3(splits), dim3(512), 0, st, d, x, in.n_rows_dev, rows, splits, part, ts);
        } else {
            if (a->dz.gmode == 0) hipLaunchKernelGGL((gemm_dw_stream_kernel<2, 0>), dim3(splits), dim3(512), 0, st, d, x, in.n_rows_dev, rows, splits, part, ts);
            else                  hipLaunchKernelGGL((gemm_dw_stream_kernel<2, 1>), dim3(splits), dim3(512), 0, st, d, x, in.n_rows_dev, rows, splits, part, ts);
        }
        GAD_CHECK_LAUNCH("gemm_dw(stream)");
        return dw_reduce_launch(part, gr, nmax, in.n_rows_dev, rows, splits, in.Kp, k_used, a->gacc, 1, st);
    }
    if (dw_wideable(*a, k_used, vec)) {
        const int tn_ = in.n_out[0] / 128, tk_ = (in.mode == 1 ? in.feat_c : in.Kp) / 128;
        int splits = gad_cdiv(g_opt.dw_wide_wgs, tn_ * tk_);             // ~one workgroup per CU
        const int by_rows = gad_cdiv(rows, 4 * KT);
        if (splits > by_rows) splits = by_rows;
        if (splits < 1) splits = 1;
        if ((long long)splits * in.n_out[0] * in.Kp <= a->partial_elems && split_on(GAD_SPLIT_DW_WIDE)) {
            // split-bf16 products: both operands are formed and split by the kernel itself (no weight mirror involved)
#define LAUNCH_DWS(XM, GM)                                                                                                     \
            hipLaunchKernelGGL((gemm_dw_wide_split_kernel<XM, GM>), dim3(tn_ * tk_, splits), dim3(256), 0, st, d, x, in.n_rows_dev, rows, \
                               in.Kp, in.n_out[0], tk_, a->partial, ts)
            if (in.mode == 1) LAUNCH_DWS(1, 0); else if (a->dz.gmode == 0) LAUNCH_DWS(0, 0); else LAUNCH_DWS(0, 1);
#undef LAUNCH_DWS
            GAD_CHECK_LAUNCH("gemm_dw(wide split)");
            return dw_reduce_launch(a->partial, gr, nmax, in.n_rows_dev, rows, splits, in.Kp, k_used, a->gacc, 0, st);
        }
        if ((long long)splits * in.n_out[0] * in.Kp <= a->partial_elems) {
            if (in.mode == 1)
                hipLaunchKernelGGL((gemm_dw_wide_kernel<1, 0>), dim3(tn_ * tk_, splits), dim3(256), 0, st, d, x, in.n_rows_dev, rows, in.Kp,
                                   in.n_out[0], tk_, a->partial, ts);
            else if (a->dz.gmode == 0)
                hipLaunchKernelGGL((gemm_dw_wide_kernel<0, 0>), dim3(tn_ * tk_, splits), dim3(256), 0, st, d, x, in.n_rows_dev, rows, in.Kp,
                                   in.n_out[0], tk_, a->partial, ts);
            else
                hipLaunchKernelGGL((gemm_dw_wide_kernel<0, 1>), dim3(tn_ * tk_, splits), dim3(256), 0, st, d, x, in.n_rows_dev, rows, in.Kp,
                                   in.n_out[0], tk_, a->partial, ts);
            GAD_CHECK_LAUNCH("gemm_dw(wide)");
            return dw_reduce_launch(a->partial, gr, nmax, in.n_rows_dev, rows, splits, in.Kp, k_used, a->gacc, 0, st);
        }
    }
    long long group_stride = 0;
#define LAUNCH_DW4(WM, WN, TM, TN, XM, V, VM)                                                              \
    hipLaunchKernelGGL((gemm_dw_kernel<WM, WN, TM, TN, XM, V, VM>), dim3(tn_ * tk_, splits, gr.n), dim3(256), 0, st, d, \
                       x, gr, in.n_rows_dev, rows, in.Kp, k_used, tk_, a->gacc, part, group_stride, ts)
#define LAUNCH_DW3(WM, WN, TM, TN, XM, V)                                                                  \
    do { if (narrow) LAUNCH_DW4(WM, WN, TM, TN, XM, V, 512); else LAUNCH_DW4(WM, WN, TM, TN, XM, V, VMAX); } while (0)
#define LAUNCH_DW(WM, WN, TM, TN)                                                                          \
    do {                                                                                                   \
        constexpr int BM = WM * TM * 32, BN = WN * TN * 32;                                                \
        const int tn_ = gad_cdiv(nmax, BM), tk_ = gad_cdiv(k_used, BN);                                    \
        splits = a->row_splits;                                                                            \
        if (splits <= 0) {                                                                                 \
            splits = gad_cdiv(512, tn_ * tk_ * gr.n);                     /* 256 / 1024 / 2048 measured slower */                                                    \
            const int by_rows = gad_cdiv(rows, 8 * KT);                                                    \
            if (splits > by_rows) splits = by_rows;                                                        \
            if (splits < 1) splits = 1;                                                                    \
        }                                                                                                  \
        group_stride = (long long)splits * nmax * in.Kp;                                                   \
        if (part && (splits == 1 || group_stride * gr.n > a->partial_elems)) part = nullptr; \
        if (g_opt.deterministic) {               /* every split's partial into the mode's zeroed slab, summed in order */ \
            part = splits > 1 ? det_dw_slab(group_stride * gr.n, stream) : nullptr;                       \
            if (splits > 1 && !part) return GAD_ERR_LAUNCH;                                                \
        }                                                                                                  \
        if (in.mode == 0) { if (vec) LAUNCH_DW3(WM, WN, TM, TN, 0, true); else LAUNCH_DW3(WM, WN, TM, TN, 0, false); } \
        else              { if (vec) LAUNCH_DW3(WM, WN, TM, TN, 1, true); else LAUNCH_DW3(WM, WN, TM, TN, 1, false); } \
    } while (0)
    int splits = 1;
    float* part = a->partial;
    const bool narrow = nmax <= 512 && (in.mode != 0 || in.c_in <= 512);   // per-channel vectors fit a 512-float stride
    if (nmax <= 32) {
        LAUNCH_DW(1, 4, 1, 1);      // 32 x 128
    } else if (k_used <= 32) {
        LAUNCH_DW(4, 1, 1, 1);      // 128 x 32
    } else {
        LAUNCH_DW(2, 2, 1, 1);      // 64 x 64
    }
#undef LAUNCH_DW
#undef LAUNCH_DW3
#undef LAUNCH_DW4
    GAD_CHECK_LAUNCH("gemm_dw");
    if (part && g_opt.deterministic) {
        for (int g = 0; g < gr.n; ++g)
            if (int e = gad_ordered_reduce(part + (size_t)g * group_stride, (long long)gr.nout[g] * in.Kp, splits,
                                           (long long)gr.nout[g] * in.Kp, a->gacc + gr.woff[g], stream)) return e;
    } else if (part) {
        return dw_reduce_launch(part, gr, nmax, in.n_rows_dev, rows, splits, in.Kp, k_used, a->gacc, 0, st);
    }
    return GAD_OK;
}

