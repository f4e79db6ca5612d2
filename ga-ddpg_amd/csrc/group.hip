// Materialising group / gather operators with their gradients, and the fused path's point layout conversion and row builders:
// gad_group_points, gad_gather_points (+ _grad), gad_prep_points, gad_rows_from_ball_query, gad_rows_group_all.
#include "common.hpp"

// ------------------------------------------------------------------------------------------------
// materialising group / gather operators (reference-API layouts, channel-major)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void group_points_kernel(const float* __restrict__ pts,
                                                           const int32_t* __restrict__ idx, int C, int N,
                                                           int MS, long long total,
                                                           float* __restrict__ out) {
    // 4 consecutive outputs per thread: one 16-B idx load, one 16-B store
    const long long q4 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (q4 >= total) return;
    const long long bc = q4 / MS;            // (b*C + c); MS % 4 == 0 is guaranteed by the host
    const int ms = (int)(q4 - bc * MS);
    const int b = (int)(bc / C);
    const int4 ii = *reinterpret_cast<const int4*>(idx + (size_t)b * MS + ms);
    const float* src = pts + (size_t)bc * N;
    float4 v = make_float4(src[ii.x], src[ii.y], src[ii.z], src[ii.w]);
    *reinterpret_cast<float4*>(out + q4) = v;
}

__global__ __launch_bounds__(256) void group_points_scalar_kernel(const float* __restrict__ pts,
                                                                  const int32_t* __restrict__ idx, int C,
                                                                  int N, int MS, long long total,
                                                                  float* __restrict__ out) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    const long long bc = q / MS;
    const int ms = (int)(q - bc * MS);
    const int b = (int)(bc / C);
    out[q] = pts[(size_t)bc * N + idx[(size_t)b * MS + ms]];
}

extern "C" int gad_group_points(const float* points, const int32_t* idx, int B, int C, int N, int M, int S,
                                float* out, void* stream) {
    GAD_REQUIRE(points && idx && out, GAD_ERR_NULL, "group_points: null pointer");
    const long long total = (long long)B * C * M * S;
    if (total == 0) return GAD_OK;
    const int MS = M * S;
    if (MS % 4 == 0) {
        hipLaunchKernelGGL(group_points_kernel, dim3(gad_cdiv(total / 4, 256)), dim3(256), 0,
                           (hipStream_t)stream, points, idx, C, N, MS, total, out);
    } else {
        hipLaunchKernelGGL(group_points_scalar_kernel, dim3(gad_cdiv(total, 256)), dim3(256), 0,
                           (hipStream_t)stream, points, idx, C, N, MS, total, out);
    }
    GAD_CHECK_LAUNCH("group_points");
    return GAD_OK;
}

__global__ __launch_bounds__(256) void group_points_grad_kernel(const float* __restrict__ go,
                                                                const int32_t* __restrict__ idx, int C,
                                                                int N, int MS, long long total,
                                                                float* __restrict__ gp) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    const long long bc = q / MS;
    const int ms = (int)(q - bc * MS);
    const int b = (int)(bc / C);
    atomic_add_f32(gp + (size_t)bc * N + idx[(size_t)b * MS + ms], go[q]);
}

// deterministic mode: one workgroup per (sample, channel) row of grad_points; thread t owns the points n = t (mod 256) of an LDS tile
// of GPG_NT points and applies the (m, s) entries that land on them in ascending order (entries staged 256 at a time).  Every
// destination is written by one thread, in entry order: the result does not depend on scheduling.  N > GPG_NT: one pass per tile.
// WEIGHTED (gad_three_interpolate_grad): entry q = i * 3 + k carries go[i] * w[q], the product rounded before it is added.
#define GPG_NT 8192
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void group_points_grad_ordered_kernel(const float* __restrict__ go, const int32_t* __restrict__ idx,
                                                                        const float* __restrict__ w, int C, int N, int MS,
                                                                        float* __restrict__ gp) {
    __shared__ float acc[GPG_NT];
    __shared__ int32_t iS[256];
    __shared__ float vS[256];
    const int bc = blockIdx.x, b = bc / C, t = threadIdx.x;
    const float* gor = go + (size_t)bc * (WEIGHTED ? MS / 3 : MS);
    const int32_t* ir = idx + (size_t)b * MS;
    for (int n0 = 0; n0 < N; n0 += GPG_NT) {
        const int nt = min(GPG_NT, N - n0);
        for (int i = t; i < nt; i += 256) acc[i] = 0.f;
        for (int q0 = 0; q0 < MS; q0 += 256) {
            __syncthreads();                             // acc cleared / the previous chunk consumed
            const int q = q0 + t;
            iS[t] = q < MS ? ir[q] - n0 : -1;
            if constexpr (WEIGHTED) vS[t] = q < MS ? gor[q / 3] * w[(size_t)b * MS + q] : 0.f;
            else vS[t] = q < MS ? gor[q] : 0.f;
            __syncthreads();
            const int nq = min(256, MS - q0);
            for (int j = 0; j < nq; ++j) {
                const int n = iS[j];
                if (n >= 0 && n < nt && (n & 255) == t) acc[n] += vS[j];
            }
        }
        __syncthreads();
        for (int i = t; i < nt; i += 256) gp[(size_t)bc * N + n0 + i] = acc[i];
    }
}
void group_points_grad_weighted_launch(const float* grad_out, const int32_t* idx, const float* weight, int B, int C, int N, int MS,
                                       float* grad_points, hipStream_t st) {
    hipLaunchKernelGGL(group_points_grad_ordered_kernel<true>, dim3(B * C), dim3(256), 0, st, grad_out, idx, weight, C, N, MS, grad_points);
}

extern "C" int gad_group_points_grad(const float* grad_out, const int32_t* idx, int B, int C, int N, int M,
                                     int S, float* grad_points, void* stream) {
    GAD_REQUIRE(grad_out && idx && grad_points, GAD_ERR_NULL, "group_points_grad: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (gad_deterministic()) {                           // (writes every element of grad_points: no clearing pass)
        if ((long long)B * C * N == 0) return GAD_OK;
        GAD_REQUIRE((long long)B * C < (1ll << 31), GAD_ERR_SHAPE, "group_points_grad: B * C too large");
        hipLaunchKernelGGL(group_points_grad_ordered_kernel<false>, dim3(B * C), dim3(256), 0, st, grad_out, idx, (const float*)nullptr, C, N,
                           M * S, grad_points);
        GAD_CHECK_LAUNCH("group_points_grad");
        return GAD_OK;
    }
    if ((long long)B * C * N > 0) { hipError_t me = hipMemsetAsync(grad_points, 0, sizeof(float) * (size_t)B * C * N, st); (void)me; }
    const long long total = (long long)B * C * M * S;
    if (total == 0) return GAD_OK;
    hipLaunchKernelGGL(group_points_grad_kernel, dim3(gad_cdiv(total, 256)), dim3(256), 0, st, grad_out, idx,
                       C, N, M * S, total, grad_points);
    GAD_CHECK_LAUNCH("group_points_grad");
    return GAD_OK;
}

extern "C" int gad_gather_points(const float* points, const int32_t* idx, int B, int C, int N, int M,
                                 float* out, void* stream) {
    // gather == group with S = 1
    return gad_group_points(points, idx, B, C, N, M, 1, out, stream);
}
extern "C" int gad_gather_points_grad(const float* grad_out, const int32_t* idx, int B, int C, int N, int M,
                                      float* grad_points, void* stream) {
    return gad_group_points_grad(grad_out, idx, B, C, N, M, 1, grad_points, stream);
}

// ------------------------------------------------------------------------------------------------
// fused-path geometry: point layout conversion and row compaction
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_points_kernel(const float* __restrict__ ps, int C4, int NP,
                                                          int skip, int N, long long total,
                                                          float* __restrict__ xyz, float* __restrict__ feat) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    const int b = (int)(q / N), j = (int)(q - (long long)b * N);
    const float* src = ps + (size_t)b * C4 * NP + skip + j;
    const float x = src[0], y = src[(size_t)NP], z = src[(size_t)2 * NP];
    const float f = C4 > 3 ? src[(size_t)3 * NP] : 0.f;
    xyz[q * 3 + 0] = x; xyz[q * 3 + 1] = y; xyz[q * 3 + 2] = z;
    *reinterpret_cast<float4*>(feat + q * 4) = make_float4(x, y, z, f);
}

extern "C" int gad_prep_points(const float* point_state, int B, int C4, int NP, int skip, float* xyz,
                               float* feat, void* stream) {
    GAD_REQUIRE(point_state && xyz && feat, GAD_ERR_NULL, "prep_points: null pointer");
    GAD_REQUIRE(C4 >= 3 && NP > skip && skip >= 0, GAD_ERR_SHAPE, "prep_points: bad shape");
    const int N = NP - skip;
    const long long total = (long long)B * N;
    if (total == 0) return GAD_OK;
    hipLaunchKernelGGL(prep_points_kernel, dim3(gad_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       point_state, C4, NP, skip, N, total, xyz, feat);
    GAD_CHECK_LAUNCH("prep_points");
    return GAD_OK;
}

// exclusive scan of max(cnt,1) over G groups by one 1024-thread workgroup, 4096 groups per pass: every thread takes four
// consecutive counts (one 16-byte load, coalesced), a wavefront scan by ds_bpermute-free shuffles, the sixteen wavefront totals
// through LDS.  (First version: every thread walked its own G / 1024 consecutive counts -- 256-byte strides between lanes -- and a
// 20-barrier Hillis-Steele pass: 101 us for the 65536 groups of configs[3]'s first module.)
__global__ __launch_bounds__(1024) void rows_scan_kernel(const int32_t* __restrict__ cnt, int G,
                                                         int32_t* __restrict__ off,
                                                         int32_t* __restrict__ n_rows) {
    __shared__ int wtot[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int run = 0;                                          // groups before this pass (uniform)
    int pass = 0;
    const bool vec = (G & 3) == 0 && ((reinterpret_cast<uintptr_t>(cnt) | reinterpret_cast<uintptr_t>(off)) & 15) == 0;
    for (int base = 0; base < G; base += 4096, ++pass) {
        const int g0 = base + 4 * tid;
        int c[4];
        if (g0 + 3 < G && vec) {
            const int4 v = *reinterpret_cast<const int4*>(cnt + g0);
            c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = g0 + i < G ? cnt[g0 + i] : 0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = g0 + i < G ? max(c[i], 1) : 0;
        const int s = c[0] + c[1] + c[2] + c[3];
        int inc = s;                                      // inclusive scan over the wavefront
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(inc, o, 64);
            if (lane >= o) inc += v;
        }
        if (lane == 63) wtot[pass & 1][wave] = inc;
        __syncthreads();                                  // (the buffer alternates: one barrier per pass)
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int t = wtot[pass & 1][w];
            before += w < wave ? t : 0;
            total += t;
        }
        int o0 = run + before + inc - s;
        if (g0 + 3 < G && vec) {
            *reinterpret_cast<int4*>(off + g0) = make_int4(o0, o0 + c[0], o0 + c[0] + c[1], o0 + c[0] + c[1] + c[2]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) { if (g0 + i < G) off[g0 + i] = o0; o0 += c[i]; }
        }
        run += total;
    }
    if (tid == 0) { off[G] = run; *n_rows = run; }
}

__global__ __launch_bounds__(256) void rows_fill_kernel(const int32_t* __restrict__ idx,
                                                        const int32_t* __restrict__ cnt,
                                                        const int32_t* __restrict__ off, int G, int M, int Nsrc,
                                                        int nsample, int32_t* __restrict__ row_pt,
                                                        int32_t* __restrict__ row_grp,
                                                        float* __restrict__ row_w) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;
    const int lane = threadIdx.x & 63;
    const int n = max(cnt[g], 1);
    const int base = off[g];
    const int b = g / M;
    for (int s = lane; s < n; s += 64) {
        row_pt[base + s] = b * Nsrc + idx[(size_t)g * nsample + s];
        row_grp[base + s] = g;
        row_w[base + s] = s == 0 ? (float)(nsample - n + 1) : 1.f;
    }
}

extern "C" int gad_rows_from_ball_query(const int32_t* idx, const int32_t* cnt, int G, int M, int Nsrc,
                                        int nsample, int32_t* grp_off, int32_t* row_pt, int32_t* row_grp,
                                        float* row_w, int32_t* n_rows, void* stream) {
    GAD_REQUIRE(idx && cnt && grp_off && row_pt && row_grp && row_w && n_rows, GAD_ERR_NULL, "rows: null pointer");
    GAD_REQUIRE(G >= 1 && M >= 1, GAD_ERR_SHAPE, "rows: bad shape");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rows_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, G, grp_off, n_rows);
    hipLaunchKernelGGL(rows_fill_kernel, dim3(gad_cdiv(G, 4)), dim3(256), 0, st, idx, cnt, grp_off, G, M, Nsrc,
                       nsample, row_pt, row_grp, row_w);
    GAD_CHECK_LAUNCH("rows_from_ball_query");
    return GAD_OK;
}

__global__ __launch_bounds__(256) void rows_group_all_kernel(int G, int P, int32_t* __restrict__ off,
                                                             int32_t* __restrict__ row_pt,
                                                             int32_t* __restrict__ row_grp,
                                                             float* __restrict__ row_w,
                                                             int32_t* __restrict__ n_rows) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < G * P) { row_pt[q] = q; row_grp[q] = q / P; row_w[q] = 1.f; }
    if (q <= G) off[q] = q * P;
    if (q == 0) *n_rows = G * P;
}

extern "C" int gad_rows_group_all(int G, int P, int32_t* grp_off, int32_t* row_pt, int32_t* row_grp,
                                  float* row_w, int32_t* n_rows, void* stream) {
    GAD_REQUIRE(grp_off && row_pt && row_grp && row_w && n_rows, GAD_ERR_NULL, "rows_group_all: null pointer");
    hipLaunchKernelGGL(rows_group_all_kernel, dim3(gad_cdiv((long long)G * P + 1, 256)), dim3(256), 0,
                       (hipStream_t)stream, G, P, grp_off, row_pt, row_grp, row_w, n_rows);
    GAD_CHECK_LAUNCH("rows_group_all");
    return GAD_OK;
}
