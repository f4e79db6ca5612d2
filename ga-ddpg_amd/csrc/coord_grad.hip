// Coordinate gradient of a set-abstraction stage's gathered first layer (gaddpg.h section C: gad_sa_coord_grad).
//
// The first 1x1 convolution of a stage reads, per row r = (group, point), the packed columns [feat | src_xyz[pt] - ctr_xyz[grp] |
// action].  gad_gemm_dx's scatter epilogue returns the feature and action columns of dZ * W and skips the three coordinate columns
// in between; this unit forms exactly those three,
//     t[r][k] = sum_c dZ[r][c] * W[c * Kp + col0 + k],   dZ[r][c] = P[c] * g - w[r] * fmaf(S[c], z, Q[c])
// (gemm_common.hpp dz_finish / dz_scalar4: the same expression on the same operands), and scatters them to where upstream's
// grouping_operation / gather_operation backward would: + t to the row's point, - t to the group's centroid point.
//
// Not a GEMM: 3 output columns over n_out channels is 6 FLOP per 8 bytes of G and z -- memory-bound, so the MFMA family is left
// alone and the shape follows the traffic instead.  A power-of-two sub-group of L = min(64, n_out / 4) lanes owns a row and reads
// it as float4s (a wavefront instruction then covers 64 / L whole rows: contiguous 16-byte pieces, not 64 lines); the 3 * n_out
// weights and P / Q / S sit in LDS, staged once per workgroup; a butterfly over the sub-group leaves the three sums in every one
// of its lanes, and lanes 0..2 issue the row's three adds on dxyz (12 contiguous bytes).  The centroid sums would put every row of
// a group on the same 12 bytes (same-address float atomics run an order of magnitude below the spread rate), so they are first
// summed per run of equal row_grp inside the wavefront -- rows of a group are contiguous -- and the run's last row adds once.
// A second, tiny launch behind the first moves the per-group sums (and the incoming gradient of new_xyz) to the centroid points;
// it must use atomics as well: several groups may share a centroid point (npoint > N, all-skipped clouds).
#include "common.hpp"

namespace {

#define CG_THREADS 256
#define CG_MAX_C 1024          // channels of the layer (6 floats of LDS each)

struct CgArgs {
    const float* z; int z_pitch;
    const float* G; int g_pitch;
    const float* P; const float* Q; const float* S;      // all three, or none (dZ = G)
    const float* row_w;
    const float* W; int Kp; int n_out; int col0;
    const int32_t* n_rows_dev; int n_rows;
    const int32_t* row_pt; const int32_t* row_grp;
    int n_groups; int n_points;
    float* dxyz; float* dctr;
    int lanes;                                           // lanes per row: a power of two, 1..64
};

// dZ of one channel (gemm_common.hpp dz_finish, the coef branch)
__device__ __forceinline__ float cg_dz(float g, float z, float w, float P, float Q, float S) { return P * g - w * fmaf(S, z, Q); }

template <bool VEC>
__global__ __launch_bounds__(CG_THREADS) void coord_grad_kernel(const CgArgs a) {
    extern __shared__ float4 cg_lds4[];                  // [W k=0 | W k=1 | W k=2 | P | Q | S], n_out floats each
    float* const lds = reinterpret_cast<float*>(cg_lds4);
    const int C = a.n_out, t = threadIdx.x;
    for (int i = t; i < C; i += CG_THREADS) {
        const float* wr = a.W + (size_t)i * a.Kp + a.col0;
        lds[i] = wr[0]; lds[C + i] = wr[1]; lds[2 * C + i] = wr[2];
        lds[3 * C + i] = a.P ? a.P[i] : 1.f;
        lds[4 * C + i] = a.P ? a.Q[i] : 0.f;
        lds[5 * C + i] = a.P ? a.S[i] : 0.f;
    }
    __syncthreads();
    int n = a.n_rows_dev ? *a.n_rows_dev : a.n_rows;
    n = n < a.n_rows ? n : a.n_rows;                     // (never beyond the static count the buffers were sized for)
    const int L = a.lanes, lane = t & 63, sub = lane & (L - 1);
    const int rows_per_wave = 64 / L, rows_per_block = CG_THREADS / L;
    const int units = VEC ? C / 4 : C;                   // float4s (VEC) or floats of a row
    const bool coef = a.P != nullptr;
    // grid-stride over slabs of rows_per_block rows; the bound is wavefront-uniform (every lane takes part in the shuffles)
    for (long long base = (long long)blockIdx.x * rows_per_block + (t >> 6) * rows_per_wave; base < n;
         base += (long long)gridDim.x * rows_per_block) {
        const long long r = base + lane / L;
        const bool live = r < n;
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
        int pt = -1, grp = -1;
        if (live) {
            const float w = a.row_w ? a.row_w[r] : 1.f;
            pt = a.row_pt[r];
            if (a.row_grp) grp = a.row_grp[r];
            for (int u = sub; u < units; u += L) {
                if constexpr (VEC) {
                    const float4 g = *reinterpret_cast<const float4*>(a.G + (size_t)r * a.g_pitch + 4 * u);
                    float4 d = g;
                    if (coef) {
                        const float4 z = *reinterpret_cast<const float4*>(a.z + (size_t)r * a.z_pitch + 4 * u);
                        const float4 P = cg_lds4[(3 * C) / 4 + u], Q = cg_lds4[(4 * C) / 4 + u], S = cg_lds4[(5 * C) / 4 + u];
                        d.x = cg_dz(g.x, z.x, w, P.x, Q.x, S.x); d.y = cg_dz(g.y, z.y, w, P.y, Q.y, S.y);
                        d.z = cg_dz(g.z, z.z, w, P.z, Q.z, S.z); d.w = cg_dz(g.w, z.w, w, P.w, Q.w, S.w);
                    }
                    const float4 w0 = cg_lds4[u], w1 = cg_lds4[C / 4 + u], w2 = cg_lds4[(2 * C) / 4 + u];
                    t0 = fmaf(d.x, w0.x, t0); t0 = fmaf(d.y, w0.y, t0); t0 = fmaf(d.z, w0.z, t0); t0 = fmaf(d.w, w0.w, t0);
                    t1 = fmaf(d.x, w1.x, t1); t1 = fmaf(d.y, w1.y, t1); t1 = fmaf(d.z, w1.z, t1); t1 = fmaf(d.w, w1.w, t1);
                    t2 = fmaf(d.x, w2.x, t2); t2 = fmaf(d.y, w2.y, t2); t2 = fmaf(d.z, w2.z, t2); t2 = fmaf(d.w, w2.w, t2);
                } else {
                    float d = a.G[(size_t)r * a.g_pitch + u];
                    if (coef) d = cg_dz(d, a.z[(size_t)r * a.z_pitch + u], w, lds[3 * C + u], lds[4 * C + u], lds[5 * C + u]);
                    t0 = fmaf(d, lds[u], t0); t1 = fmaf(d, lds[C + u], t1); t2 = fmaf(d, lds[2 * C + u], t2);
                }
            }
        }
        for (int o = L >> 1; o >= 1; o >>= 1) {          // butterfly inside the row's sub-group: every lane ends with the sums
            t0 += __shfl_xor(t0, o, 64); t1 += __shfl_xor(t1, o, 64); t2 += __shfl_xor(t2, o, 64);
        }
        // a row whose point (group) number lies outside the buffers is skipped, never written through
        const bool pt_ok = live && (unsigned)pt < (unsigned)a.n_points;
        if (pt_ok)
            for (int k = sub; k < 3; k += L) atomic_add_f32(a.dxyz + (size_t)pt * 3 + k, k == 0 ? t0 : (k == 1 ? t1 : t2));
        if (a.row_grp) {                                 // (kernel-argument uniform)
            if (!pt_ok) t0 = t1 = t2 = 0.f;
            // segmented inclusive scan over the wavefront's rows, a run = consecutive rows of one group (head flags, so a row list
            // that broke the contiguity contract would cost adds, not correctness); the last row of each run adds the run's sum
            const int pg = __shfl_up(grp, L, 64);        // (every lane executes the shuffle: an inactive source lane reads as 0)
            int head = (lane < L || pg != grp) ? 1 : 0;
            for (int d = L; d < 64; d <<= 1) {
                const int oh = __shfl_up(head, d, 64);
                const float u0 = __shfl_up(t0, d, 64), u1 = __shfl_up(t1, d, 64), u2 = __shfl_up(t2, d, 64);
                if (lane >= d) {
                    if (!head) { t0 += u0; t1 += u1; t2 += u2; }
                    head |= oh;
                }
            }
            const int ng = __shfl_down(grp, L, 64);
            const bool last = lane + L >= 64 || ng != grp;
            if ((unsigned)grp < (unsigned)a.n_groups && last)
                for (int k = sub; k < 3; k += L) atomic_add_f32(a.dctr + (size_t)grp * 3 + k, k == 0 ? t0 : (k == 1 ? t1 : t2));
        }
    }
}

// dxyz[ctr_pt[g]][k] += g_new_xyz[g][k] - dctr[g][k]: the centroid is subtracted from every row of its group, and new_xyz is a
// gather of the centroid points
__global__ __launch_bounds__(CG_THREADS) void coord_grad_centroid_kernel(const int32_t* __restrict__ ctr_pt, const float* __restrict__ g_new_xyz,
                                                                         const float* __restrict__ dctr, int n_groups, int n_points,
                                                                         float* __restrict__ dxyz) {
    const int total = n_groups * 3;
    for (int i = blockIdx.x * CG_THREADS + threadIdx.x; i < total; i += gridDim.x * CG_THREADS) {
        const int g = i / 3, k = i - 3 * g;
        const int pt = ctr_pt[g];
        if ((unsigned)pt >= (unsigned)n_points) continue;
        const float up = g_new_xyz ? g_new_xyz[i] : 0.f;
        atomic_add_f32(dxyz + (size_t)pt * 3 + k, up - dctr[i]);
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

}        // namespace

extern "C" int gad_sa_coord_grad(const gad_dz_src* dz, const float* W, int Kp, int n_out, int col0, const int32_t* n_rows_dev,
                                 int n_rows, const int32_t* row_pt, const int32_t* row_grp, const int32_t* ctr_pt,
                                 const float* g_new_xyz, int n_groups, int n_points, float* dxyz, float* dctr, void* stream) {
    GAD_REQUIRE(dz && W && row_pt && dxyz, GAD_ERR_NULL, "sa_coord_grad: null dz / W / row_pt / dxyz");
    GAD_REQUIRE(Kp >= 0 && n_out >= 0 && col0 >= 0 && n_rows >= 0 && n_groups >= 0 && n_points >= 0, GAD_ERR_SHAPE,
                "sa_coord_grad: negative size (Kp %d, n_out %d, col0 %d, n_rows %d, groups %d, points %d)", Kp, n_out, col0, n_rows,
                n_groups, n_points);
    GAD_REQUIRE(n_out >= 1 && n_out <= CG_MAX_C, GAD_ERR_SHAPE, "sa_coord_grad: n_out %d outside 1..%d", n_out, CG_MAX_C);
    GAD_REQUIRE(Kp >= col0 + 3, GAD_ERR_SHAPE, "sa_coord_grad: Kp %d holds no three coordinate columns from col0 %d", Kp, col0);
    GAD_REQUIRE(dz->gmode == 0 && dz->G, GAD_ERR_NULL, "sa_coord_grad: the first layer's gradient source is a dense G (gmode 0)");
    GAD_REQUIRE(dz->c == n_out && dz->g_pitch >= n_out, GAD_ERR_SHAPE, "sa_coord_grad: dz.c %d / g_pitch %d against n_out %d", dz->c,
                dz->g_pitch, n_out);
    GAD_REQUIRE(dz->premasked || !dz->relu, GAD_ERR_UNSUPPORTED, "sa_coord_grad: G must carry the ReLU mask already (premasked)");
    GAD_REQUIRE(!dz->bn_dbeta, GAD_ERR_UNSUPPORTED, "sa_coord_grad: coefP / Q / S are read as given (no bn_* block)");
    const bool coef = dz->coefP != nullptr;
    GAD_REQUIRE(coef == (dz->coefQ != nullptr) && coef == (dz->coefS != nullptr), GAD_ERR_NULL,
                "sa_coord_grad: coefP / coefQ / coefS are given together or not at all");
    GAD_REQUIRE(!coef || (dz->z && dz->z_pitch >= n_out), GAD_ERR_NULL, "sa_coord_grad: BatchNorm coefficients need z (pitch >= n_out)");
    GAD_REQUIRE(!row_grp || (ctr_pt && dctr), GAD_ERR_NULL, "sa_coord_grad: row_grp without centroid points / dctr");
    GAD_REQUIRE(!ctr_pt || row_grp, GAD_ERR_NULL, "sa_coord_grad: centroid points without row_grp");
    GAD_REQUIRE(!g_new_xyz || ctr_pt, GAD_ERR_NULL, "sa_coord_grad: g_new_xyz without centroid points");
    if (n_rows == 0 || n_groups == 0) return GAD_OK;
    GAD_REQUIRE((long long)n_groups * 3 < (1ll << 31) && (long long)n_points * 3 < (1ll << 31), GAD_ERR_SHAPE,
                "sa_coord_grad: %d groups / %d points overflow 32-bit element indices", n_groups, n_points);
    GAD_REQUIRE(!gad_deterministic(), GAD_ERR_UNSUPPORTED,
                "sa_coord_grad: option \"deterministic\" is set and the scatter uses float atomics (no ordered form)");
    CgArgs a;
    a.z = dz->z; a.z_pitch = dz->z_pitch; a.G = dz->G; a.g_pitch = dz->g_pitch;
    a.P = dz->coefP; a.Q = dz->coefQ; a.S = dz->coefS; a.row_w = dz->row_w;
    a.W = W; a.Kp = Kp; a.n_out = n_out; a.col0 = col0;
    a.n_rows_dev = n_rows_dev; a.n_rows = n_rows; a.row_pt = row_pt; a.row_grp = row_grp;
    a.n_groups = n_groups; a.n_points = n_points; a.dxyz = dxyz; a.dctr = dctr;
    const bool vec = n_out % 4 == 0 && dz->g_pitch % 4 == 0 && aligned16(dz->G) &&
                     (!coef || (dz->z_pitch % 4 == 0 && aligned16(dz->z)));
    const int units = vec ? n_out / 4 : n_out;
    int L = 1;
    while (L * 2 <= units && L < 64) L *= 2;
    a.lanes = L;
    const int rows_per_block = CG_THREADS / L;
    int blocks = gad_cdiv(n_rows, rows_per_block);
    if (blocks > 2048) blocks = 2048;                    // 8 workgroups on each of the 256 CUs; the loop strides over the rest
    const size_t lds = sizeof(float) * 6 * (size_t)n_out;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(coord_grad_kernel<true>, dim3(blocks), dim3(CG_THREADS), lds, st, a);
    else hipLaunchKernelGGL(coord_grad_kernel<false>, dim3(blocks), dim3(CG_THREADS), lds, st, a);
    GAD_CHECK_LAUNCH("sa_coord_grad");
    if (ctr_pt) {
        int cb = gad_cdiv((long long)n_groups * 3, CG_THREADS);
        if (cb > 1024) cb = 1024;
        hipLaunchKernelGGL(coord_grad_centroid_kernel, dim3(cb), dim3(CG_THREADS), 0, st, ctr_pt, g_new_xyz, dctr, n_groups, n_points, dxyz);
        GAD_CHECK_LAUNCH("sa_coord_grad(centroids)");
    }
    return GAD_OK;
}
