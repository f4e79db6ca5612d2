// Feature propagation on the layer-GEMM family (gaddpg.h section C.2): what a PointnetFPModule needs around gad_gemm_fwd / _dx / _dw
// over dense rows -- the row matrix at the module's entry (gad_fp_rows: three_interpolate written as GEMM input rows, and its
// gradient gad_fp_rows_grad) and the activation at its exit (gad_rows_act_out: BatchNorm affine + ReLU with the transpose to
// upstream's (B, C, n) folded in, and gad_rows_act_bwd_stats: the ReLU-masked incoming gradient as rows with the last layer's
// dbeta / dgamma sums).  For a set-abstraction stage the gather and the max-pool stand in these places.
// Upstream code replaced: three_interpolate + torch.cat + SharedMLP of pointnet2_modules.PointnetFPModule.forward.
#include "common.hpp"

// ------------------------------------------------------------------------------------------------
// gad_fp_rows: rows[b * n + i][off + c] = (w0 * f[j0][c] + w1 * f[j1][c]) + w2 * f[j2][c]
// ------------------------------------------------------------------------------------------------
// A neighbour's channels are contiguous in the point-major source, so a lane takes V consecutive channels of one row (V = 4:
// 16-byte loads and stores; V = 1 where C2, a pitch, the offset or a base address does not allow them) and consecutive lanes take
// consecutive channel groups of the same row: every wave instruction reads three runs of a few rows and writes one run.  The
// three indices and weights of a row are read by each of its lanes (one cached line per row).  Every product and sum is rounded on
// its own, in three_interpolate_kernel's order: the result is that kernel's, transposed.
template <int V>
__global__ __launch_bounds__(256) void fp_rows_kernel(const float* __restrict__ known, int k_pitch, const int32_t* __restrict__ idx,
                                                      const float* __restrict__ w, int n, int m, int per_row, long long total,
                                                      float* __restrict__ rows, int r_pitch, int col_off) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    const long long r = q / per_row;
    const int c = (int)(q - r * per_row) * V;
    const long long b = r / n;
    const size_t t = (size_t)r * 3;
    const int j0 = idx[t], j1 = idx[t + 1], j2 = idx[t + 2];
    const float w0 = w[t], w1 = w[t + 1], w2 = w[t + 2];
    const float* kb = known + (size_t)b * m * k_pitch + c;
    float* dst = rows + (size_t)r * r_pitch + col_off + c;
    if (V == 4) {
        const float4 f0 = *reinterpret_cast<const float4*>(kb + (size_t)j0 * k_pitch);
        const float4 f1 = *reinterpret_cast<const float4*>(kb + (size_t)j1 * k_pitch);
        const float4 f2 = *reinterpret_cast<const float4*>(kb + (size_t)j2 * k_pitch);
        float4 o;
        { const float a0 = w0 * f0.x, a1 = w1 * f1.x, a2 = w2 * f2.x; o.x = (a0 + a1) + a2; }
        { const float a0 = w0 * f0.y, a1 = w1 * f1.y, a2 = w2 * f2.y; o.y = (a0 + a1) + a2; }
        { const float a0 = w0 * f0.z, a1 = w1 * f1.z, a2 = w2 * f2.z; o.z = (a0 + a1) + a2; }
        { const float a0 = w0 * f0.w, a1 = w1 * f1.w, a2 = w2 * f2.w; o.w = (a0 + a1) + a2; }
        *reinterpret_cast<float4*>(dst) = o;
    } else {
        const float a0 = w0 * kb[(size_t)j0 * k_pitch], a1 = w1 * kb[(size_t)j1 * k_pitch], a2 = w2 * kb[(size_t)j2 * k_pitch];
        *dst = (a0 + a1) + a2;
    }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// the shape checks the two row entry points share: sizes, the column window inside a row, 32-bit row / point counts
static int fp_rows_check(const char* who, int B, int n, int m, int C2, int k_pitch, int r_pitch, int col_off) {
    GAD_REQUIRE(B >= 0 && n >= 0 && m >= 0 && C2 >= 0, GAD_ERR_SHAPE, "%s: negative size (B %d, n %d, m %d, C2 %d)", who, B, n, m, C2);
    GAD_REQUIRE(k_pitch >= C2, GAD_ERR_SHAPE, "%s: known rows of pitch %d hold no %d channels", who, k_pitch, C2);
    GAD_REQUIRE(col_off >= 0 && (long long)col_off + C2 <= r_pitch, GAD_ERR_SHAPE, "%s: columns [%d, %d + %d) outside a row of pitch %d", who,
                col_off, col_off, C2, r_pitch);
    GAD_REQUIRE((long long)B * n < (1ll << 31) && (long long)B * m < (1ll << 31), GAD_ERR_SHAPE, "%s: B * n or B * m too large (B %d, n %d, m %d)",
                who, B, n, m);
    return GAD_OK;
}

extern "C" int gad_fp_rows(const float* known_pm, int k_pitch, const int32_t* idx, const float* weight, int B, int n, int m, int C2,
                           float* rows, int r_pitch, int col_off, void* stream) {
    GAD_REQUIRE(known_pm && idx && weight && rows, GAD_ERR_NULL, "fp_rows: null pointer");
    if (int e = fp_rows_check("fp_rows", B, n, m, C2, k_pitch, r_pitch, col_off)) return e;
    if ((long long)B * n * C2 == 0) return GAD_OK;
    GAD_REQUIRE(m >= 1, GAD_ERR_SHAPE, "fp_rows: no known point (m = %d) for %d points", m, n);
    const bool v4 = C2 % 4 == 0 && k_pitch % 4 == 0 && r_pitch % 4 == 0 && col_off % 4 == 0 && aligned16(known_pm) && aligned16(rows);
    const int per_row = v4 ? C2 / 4 : C2;
    const long long total = (long long)B * n * per_row;
    GAD_REQUIRE((total + 255) / 256 < (1ll << 31), GAD_ERR_SHAPE, "fp_rows: B * n * C2 too large");
    const dim3 grid((unsigned)((total + 255) / 256));
    if (v4)
        hipLaunchKernelGGL(fp_rows_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, known_pm, k_pitch, idx, weight, n, m, per_row, total,
                           rows, r_pitch, col_off);
    else
        hipLaunchKernelGGL(fp_rows_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, known_pm, k_pitch, idx, weight, n, m, per_row, total,
                           rows, r_pitch, col_off);
    GAD_CHECK_LAUNCH("fp_rows");
    return GAD_OK;
}

// ------------------------------------------------------------------------------------------------
// gad_fp_rows_grad: gknown[b * m + j_k][c] += w_k * drows[r][off + c]
// ------------------------------------------------------------------------------------------------
// One lane per (row, channel), consecutive lanes = consecutive channels of the row: each of the three atomic instructions of a
// wavefront adds into contiguous channels of one destination row (of two or more rows where C2 < 64).  The order of the adds into
// an element is the hardware's: there is no ordered form here, the deterministic mode is refused before any launch.
__global__ __launch_bounds__(256) void fp_rows_grad_kernel(const float* __restrict__ drows, int r_pitch, int col_off,
                                                           const int32_t* __restrict__ idx, const float* __restrict__ w, int n, int m,
                                                           int C2, long long total, float* __restrict__ gk, int k_pitch) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    const long long r = q / C2;
    const int c = (int)(q - r * C2);
    const long long b = r / n;
    const size_t t = (size_t)r * 3;
    const int j0 = idx[t], j1 = idx[t + 1], j2 = idx[t + 2];
    const float w0 = w[t], w1 = w[t + 1], w2 = w[t + 2];
    const float g = drows[(size_t)r * r_pitch + col_off + c];
    float* d = gk + (size_t)b * m * k_pitch + c;
    atomic_add_f32(d + (size_t)j0 * k_pitch, g * w0);
    atomic_add_f32(d + (size_t)j1 * k_pitch, g * w1);
    atomic_add_f32(d + (size_t)j2 * k_pitch, g * w2);
}

extern "C" int gad_fp_rows_grad(const float* drows, int r_pitch, int col_off, const int32_t* idx, const float* weight, int B, int n,
                                int m, int C2, float* gknown_pm, int k_pitch, void* stream) {
    GAD_REQUIRE(drows && idx && weight && gknown_pm, GAD_ERR_NULL, "fp_rows_grad: null pointer");
    if (int e = fp_rows_check("fp_rows_grad", B, n, m, C2, k_pitch, r_pitch, col_off)) return e;
    GAD_REQUIRE(!gad_deterministic(), GAD_ERR_UNSUPPORTED, "fp_rows_grad: float atomics, no ordered form (option \"deterministic\"): "
                "transpose the row gradient and call gad_three_interpolate_grad");
    if ((long long)B * n * C2 == 0) return GAD_OK;
    GAD_REQUIRE(m >= 1, GAD_ERR_SHAPE, "fp_rows_grad: no known point (m = %d) for %d points", m, n);
    const long long total = (long long)B * n * C2;
    GAD_REQUIRE((total + 255) / 256 < (1ll << 31), GAD_ERR_SHAPE, "fp_rows_grad: B * n * C2 too large");
    hipLaunchKernelGGL(fp_rows_grad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, drows, r_pitch,
                       col_off, idx, weight, n, m, C2, total, gknown_pm, k_pitch);
    GAD_CHECK_LAUNCH("fp_rows_grad");
    return GAD_OK;
}

// ------------------------------------------------------------------------------------------------
// gad_rows_act_out: out[b][c][i] = relu(fma(z[b * n + i][c], scale[c], shift[c]))
// ------------------------------------------------------------------------------------------------
// gad_affine_act's arithmetic with gad_transpose_batched's 32 x 33 LDS tile behind it: 128-byte row segments of z in, 128-byte
// segments of a channel's points out.  Workgroup = (sample, 32 points) x 32 channels.
__global__ __launch_bounds__(256) void rows_act_out_kernel(const float* __restrict__ z, int z_pitch, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, int n, int C, int ptiles,
                                                           float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int b = blockIdx.x / ptiles, i0 = (blockIdx.x - b * ptiles) * 32, c0 = blockIdx.y * 32;
    const int c = c0 + tx;
    float sc = 0.f, sh = 0.f;
    if (c < C) { sc = scale[c]; sh = shift[c]; }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = i0 + ty + 8 * u;
        if (i < n && c < C) tile[ty + 8 * u][tx] = fmaxf(fmaf(z[((size_t)b * n + i) * z_pitch + c], sc, sh), 0.f);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int cc = c0 + ty + 8 * u, i = i0 + tx;
        if (i < n && cc < C) out[((size_t)b * C + cc) * n + i] = tile[tx][ty + 8 * u];
    }
}

extern "C" int gad_rows_act_out(const float* z, int z_pitch, const float* scale, const float* shift, int B, int n, int C, float* out,
                                void* stream) {
    GAD_REQUIRE(z && scale && shift && out, GAD_ERR_NULL, "rows_act_out: null pointer");
    GAD_REQUIRE(B >= 0 && n >= 0 && C >= 0 && z_pitch >= C, GAD_ERR_SHAPE, "rows_act_out: B=%d n=%d C=%d, row pitch %d (rows would overlap)", B,
                n, C, z_pitch);
    if ((long long)B * n * C == 0) return GAD_OK;
    const int ptiles = gad_cdiv(n, 32);
    GAD_REQUIRE((long long)B * ptiles < (1ll << 31) && gad_cdiv(C, 32) <= 65535, GAD_ERR_SHAPE, "rows_act_out: B * n or C too large");
    hipLaunchKernelGGL(rows_act_out_kernel, dim3((unsigned)(B * ptiles), gad_cdiv(C, 32)), dim3(256), 0, (hipStream_t)stream, z, z_pitch,
                       scale, shift, n, C, ptiles, out);
    GAD_CHECK_LAUNCH("rows_act_out");
    return GAD_OK;
}

// ------------------------------------------------------------------------------------------------
// gad_rows_act_bwd_stats: G[r][c] = dout[b][c][i] where fma(z[r][c], scale, shift) > 0, else 0; dbeta += sum G, dgamma += sum G * x_hat
// ------------------------------------------------------------------------------------------------
// What gad_pool_bwd_stats (mask_in_place) is to a pooled layer, for a layer whose every row goes out: the transpose of the incoming
// gradient through the same LDS tile, the ReLU mask from the raw z, and the two BatchNorm-backward sums.  A workgroup owns 32
// channels and walks (sample, 32 points) tiles in a grid-stride loop; a thread keeps its channel's two sums in f64 over its rows,
// the eight row phases are folded through LDS and one f64 atomic per channel and workgroup goes to replica blockIdx.x %
// GAD_STAT_REPLICAS.  DET: the workgroup's sums are stored into its slot of a plane instead (the grid is a function of B, n and C
// alone) and gad_ordered_reduce adds the slots in order.
#define RAB_GX_CAP 512
template <bool DET>
__global__ __launch_bounds__(256) void rows_act_bwd_stats_kernel(const float* __restrict__ dout, const float* __restrict__ z, int z_pitch,
                                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                                 const float* __restrict__ mean, const float* __restrict__ istd, int n,
                                                                 int C, int ptiles, int ntiles, float* __restrict__ G, int g_pitch,
                                                                 double* __restrict__ dbeta, double* __restrict__ dgamma, int stride) {
    __shared__ float tile[32][33];
    __shared__ double red[2][8][32];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.y * 32, c = c0 + tx;
    float sc = 0.f, sh = 0.f, mu = 0.f, is = 0.f;
    if (c < C) { sc = scale[c]; sh = shift[c]; mu = mean[c]; is = istd[c]; }
    double sb = 0.0, sg = 0.0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int b = t / ptiles, i0 = (t - b * ptiles) * 32;
        __syncthreads();                                  // the previous tile consumed
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int cc = c0 + ty + 8 * u, i = i0 + tx;
            tile[ty + 8 * u][tx] = (i < n && cc < C) ? dout[((size_t)b * C + cc) * n + i] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + ty + 8 * u;
            if (i < n && c < C) {
                const size_t r = (size_t)b * n + i;
                const float zv = z[r * z_pitch + c];
                const bool live = fmaf(zv, sc, sh) > 0.f;
                const float g = live ? tile[tx][ty + 8 * u] : 0.f;
                G[r * g_pitch + c] = g;
                if (live) {
                    sb += (double)g;
                    sg += (double)g * (((double)zv - (double)mu) * (double)is);
                }
            }
        }
    }
    red[0][ty][tx] = sb;
    red[1][ty][tx] = sg;
    __syncthreads();
    if (ty == 0 && c < C) {
        double b0 = 0.0, g0 = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) { b0 += red[0][k][tx]; g0 += red[1][k][tx]; }
        if (DET) {
            dbeta[(size_t)blockIdx.x * stride + c] = b0;
            dgamma[(size_t)blockIdx.x * stride + c] = g0;
        } else {
            const int rep = blockIdx.x % GAD_STAT_REPLICAS;
            atomic_add_f64(dbeta + (size_t)rep * stride + c, b0);
            atomic_add_f64(dgamma + (size_t)rep * stride + c, g0);
        }
    }
}

extern "C" int gad_rows_act_bwd_stats(const float* dout, const float* z, int z_pitch, const float* scale, const float* shift,
                                      const float* mean, const float* istd, int B, int n, int C, float* G, int g_pitch, double* dbeta,
                                      double* dgamma, int stat_stride, void* stream) {
    GAD_REQUIRE(dout && z && scale && shift && mean && istd && G && dbeta && dgamma, GAD_ERR_NULL, "rows_act_bwd_stats: null pointer");
    GAD_REQUIRE(B >= 0 && n >= 0 && C >= 0 && z_pitch >= C && g_pitch >= C, GAD_ERR_SHAPE,
                "rows_act_bwd_stats: B=%d n=%d C=%d, row pitches %d / %d (rows would overlap)", B, n, C, z_pitch, g_pitch);
    if ((long long)B * n * C == 0) return GAD_OK;
    GAD_REQUIRE(stat_stride >= C, GAD_ERR_SHAPE, "rows_act_bwd_stats: stat_stride %d < C %d (the replicas would overlap)", stat_stride, C);
    const int ptiles = gad_cdiv(n, 32);
    GAD_REQUIRE((long long)B * ptiles < (1ll << 31) && gad_cdiv(C, 32) <= 65535, GAD_ERR_SHAPE, "rows_act_bwd_stats: B * n or C too large");
    const int ntiles = B * ptiles;
    const int gx = ntiles < RAB_GX_CAP ? ntiles : RAB_GX_CAP;
    const dim3 grid(gx, gad_cdiv(C, 32));
    hipStream_t st = (hipStream_t)stream;
    if (gad_deterministic()) {                            // (gx depends on B, n and C only: the same slots in every run)
        double* slots = static_cast<double*>(gad_det_scratch(stream, GAD_DET_SLOTS, 2 * (size_t)gx * C * sizeof(double)));
        if (!slots) return GAD_ERR_LAUNCH;
        hipLaunchKernelGGL(rows_act_bwd_stats_kernel<true>, grid, dim3(256), 0, st, dout, z, z_pitch, scale, shift, mean, istd, n, C, ptiles,
                           ntiles, G, g_pitch, slots, slots + (size_t)gx * C, C);
        GAD_CHECK_LAUNCH("rows_act_bwd_stats");
        if (int e = gad_ordered_reduce(slots, C, gx, C, dbeta, stream)) return e;
        return gad_ordered_reduce(slots + (size_t)gx * C, C, gx, C, dgamma, stream);
    }
    hipLaunchKernelGGL(rows_act_bwd_stats_kernel<false>, grid, dim3(256), 0, st, dout, z, z_pitch, scale, shift, mean, istd, n, C, ptiles,
                       ntiles, G, g_pitch, dbeta, dgamma, stat_stride);
    GAD_CHECK_LAUNCH("rows_act_bwd_stats");
    return GAD_OK;
}
