// Fused backward of the layer-GEMM family (overview and map of the units: gemm.hip): the SA1 streaming backward kernels (streaming dX,
// fused dX + dW and their split form), the fused wide backward, their route predicates, gad_gemm_bwd and gad_gemm_dw_reduce.
#include "gemm_common.hpp"

// ------------------------------------------------------------------------------------------------
// streaming dX for the SA1 layers (rows ~ 2e5, n_out in {64,128} reduced onto 64 input channels): the backward twin
// of gemm_fwd_stream_kernel.  HBM-bound (1 KB per row: z and dY in, dY out, z_prev for the BatchNorm-backward sums).
//   * W^T staged once per workgroup in LDS ([k][n_out+4]: B fragments are conflict-free ds_read_b128);
//   * the A operand dZ[r][8j+4h..+3] is produced in registers from 16-byte loads of z and dY (or of the pooled
//     arg-max / gradient pair), four k-groups per register chunk, the next chunk (or the next slab's first chunk)
//     in flight during the current chunk's MFMAs;
//   * epilogue: dY of the previous layer through buffer stores (SGPR row offsets) + that layer's dbeta / dgamma sums;
//     its z_prev loads are issued before the last chunk's MFMAs.
// ------------------------------------------------------------------------------------------------
template <int NJ, int GM>
__global__ __launch_bounds__(512, 2) void gemm_dx_stream_kernel(DzSrc d, const int32_t* __restrict__ n_rows_dev,
                                                                 int n_rows_static, const float* __restrict__ W, DxEpi e, unsigned long long* __restrict__ ts) {
    KTimer kt(ts);
    constexpr int NO = 8 * NJ, PW = NO + 4, NCH = NJ / 4;
    __shared__ __attribute__((aligned(16))) float Wt[64 * PW];
    __shared__ __attribute__((aligned(16))) float vec[3 * NO];          // P | Q | S (the ReLU mask is already in dY: premasked)
    __shared__ float red[2 * 8 * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    {   // W (n_out x 64, row-major) -> W^T in LDS
        constexpr int UW = NO * 16 / 512;
        float4 wr[UW];
#pragma unroll
        for (int it = 0; it < UW; ++it) wr[it] = ldg4(W + (size_t)(it * 512 + tid) * 4);
#pragma unroll
        for (int it = 0; it < UW; ++it) {
            const int u = it * 512 + tid;
            const int n = u >> 4, k4 = (u & 15) * 4;
            Wt[(k4 + 0) * PW + n] = wr[it].x; Wt[(k4 + 1) * PW + n] = wr[it].y;
            Wt[(k4 + 2) * PW + n] = wr[it].z; Wt[(k4 + 3) * PW + n] = wr[it].w;
        }
    }
    for (int i = tid; i < NO; i += 512) {
        float P, Q, S;
        dz_coef(d, i, P, Q, S, first_workgroup());
        vec[i] = P; vec[NO + i] = Q; vec[2 * NO + i] = S;
    }
    __syncthreads();
    // previous layer's BatchNorm vectors of this lane's two output columns
    float ps[2], pt[2], pm[2], pi[2];
#pragma unroll
    for (int tk = 0; tk < 2; ++tk) {
        const int k = tk * 32 + l31;
        ps[tk] = e.ps[k]; pt[tk] = e.pt[k]; pm[tk] = e.pm[k]; pi[tk] = e.pi[k];
    }
    const int n_slabs = (n_rows + 31) >> 5;
    const int stride = gridDim.x * 8;
    int slab = wave * gridDim.x + blockIdx.x;                 // wave-uniform; same dealing as the forward kernel
    const __amdgpu_buffer_rsrc_t grsrc = __builtin_amdgcn_make_buffer_rsrc(e.gout, 0, gad_nbytes(n_rows, 64 * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t zrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(e.zprev), 0, gad_nbytes(n_rows_static, 64 * 4), 0x00020000);
    const int glane = (4 * half * 64 + l31) * 4;

    float sb[2] = {0.f, 0.f}, sg[2] = {0.f, 0.f};
    float4 rz[2][4], rg[2][4];
    int4 ra[2][4];
    auto row_of = [&](int sl) { return min(sl < n_slabs ? sl * 32 + l31 : 0, max(n_rows - 1, 0)); };
    auto load_chunk = [&](int r, int grp, int c, int buf) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned n = 8 * (4 * c + u) + 4 * half;
            rz[buf][u] = ldg4(d.z + ((unsigned)r * NO + n));
            if (GM == 0) {
                rg[buf][u] = ldg4(d.G + ((unsigned)r * NO + n));
            } else {
                ra[buf][u] = *reinterpret_cast<const int4*>(d.argmax + ((unsigned)grp * NO + n));
                rg[buf][u] = ldg4(d.dout + ((unsigned)grp * NO + n));
            }
        }
    };
    int r_cur = row_of(slab);
    int grp_cur = GM == 1 ? d.row_grp[r_cur] : 0;
    load_chunk(r_cur, grp_cur, 0, 0);
    for (; slab < n_slabs; slab += stride) {
        const int r_nxt = row_of(slab + stride);
        const int grp_nxt = GM == 1 ? d.row_grp[r_nxt] : 0;
        const float wrow = d.row_w ? d.row_w[r_cur] : 1.f;
        __asm__ volatile("" ::: "memory");            // keep loop-invariant LDS reads inside the loop (registers)
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
        float zp[2][16];
        const int zrow = slab * 32 * 64 * 4;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (c + 1 < NCH) load_chunk(r_cur, grp_cur, c + 1, (c + 1) & 1);
            else {
                load_chunk(r_nxt, grp_nxt, 0, 0);
#pragma unroll
                for (int v = 0; v < 16; ++v)
#pragma unroll
                    for (int t = 0; t < 2; ++t)
                        zp[t][v] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                            zrsrc, glane + t * 128, zrow + ((v & 3) + 8 * (v >> 2)) * 256, 0));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int n = 8 * (4 * c + u) + 4 * half;
                const float4 z = rz[c & 1][u];
                float4 g = rg[c & 1][u];
                if (GM == 1) {
                    const int4 a = ra[c & 1][u];
                    const int rr = slab * 32 + l31;                 // true row (clamped rows never match: rr >= n_rows > any arg-max)
                    g.x = a.x == rr ? g.x : 0.f; g.y = a.y == rr ? g.y : 0.f;
                    g.z = a.z == rr ? g.z : 0.f; g.w = a.w == rr ? g.w : 0.f;
                }
                const float4 P = *reinterpret_cast<const float4*>(vec + n);
                const float4 Q = *reinterpret_cast<const float4*>(vec + NO + n);
                const float4 S = *reinterpret_cast<const float4*>(vec + 2 * NO + n);
                float4 a4;
                a4.x = P.x * g.x - wrow * fmaf(S.x, z.x, Q.x); a4.y = P.y * g.y - wrow * fmaf(S.y, z.y, Q.y);
                a4.z = P.z * g.z - wrow * fmaf(S.z, z.z, Q.z); a4.w = P.w * g.w - wrow * fmaf(S.w, z.w, Q.w);
                const float4 b0 = *reinterpret_cast<const float4*>(Wt + l31 * PW + n);
                const float4 b1 = *reinterpret_cast<const float4*>(Wt + (32 + l31) * PW + n);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b0.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b1.x, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b0.y, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b1.y, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b0.z, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b1.z, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b0.w, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b1.w, acc[1], 0, 0, 0);
            }
        }
        // epilogue: dY of the previous layer + its BatchNorm-backward sums (rows past n_rows: the store is dropped by
        // the buffer bounds only for the voffset part, so ragged slabs are predicated; their sums are masked)
        const bool full = slab * 32 + 32 <= n_rows;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int row = acc_row(v, half);
            const bool live = slab * 32 + row < n_rows;
            const int rb = zrow + ((v & 3) + 8 * (v >> 2)) * 256;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float gv = acc[t][v];
                const float zv = live ? zp[t][v] : 0.f;       // rows past n_rows hold whatever the allocation held (NaN x 0 = NaN)
                const bool act = fmaf(zv, ps[t], pt[t]) > 0.f && live;
                const float ga = act ? gv : 0.f;
                // the previous layer's consumers take dY with its ReLU mask applied (premasked)
                if (full) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ga), grsrc, glane + t * 128, rb, GAD_STREAM_STORE_AUX);
                else if (live) e.gout[(size_t)(slab * 32 + row) * 64 + t * 32 + l31] = ga;
                sb[t] += ga;
                sg[t] = fmaf(ga, (zv - pm[t]) * pi[t], sg[t]);
            }
        }
        r_cur = r_nxt;
        grp_cur = grp_nxt;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float s0 = sb[t] + __shfl_xor(sb[t], 32, 64);
        const float s1 = sg[t] + __shfl_xor(sg[t], 32, 64);
        if (lane < 32) { red[wave * 64 + t * 32 + lane] = s0; red[(8 + wave) * 64 + t * 32 + lane] = s1; }
    }
    __syncthreads();
    if (tid < 64) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) { s0 += red[w * 64 + tid]; s1 += red[(8 + w) * 64 + tid]; }
        const int rep = blockIdx.x % GAD_STAT_REPLICAS;
        atomic_add_f64(e.dbeta + (size_t)rep * e.stat_stride + tid, (double)s0);
        atomic_add_f64(e.dgamma + (size_t)rep * e.stat_stride + tid, (double)s1);
    }
}

// ------------------------------------------------------------------------------------------------
// Fused backward of an SA1 layer (rows ~ 2e5, 64 input channels, 64 / 128 output channels): dX AND dW in one pass over
// z / dY / z_prev.  The two streaming kernels above read the same 55 - 110 MB tensors from two streams at once and slow each
// other down far below what either reaches alone (layer 3: 67 + 83 us alone, 119 + 168 us side by side).  Here a workgroup
// of 8 wavefronts splits into 4 PRODUCERS and 4 CONSUMERS (one of each per SIMD, so the MFMA pipe of a SIMD alternates
// between them) and walks quads of four 32-row slabs:
//   producer p takes slab 4*quad + p exactly as gemm_dx_stream_kernel does (16-byte loads of z and dY, dZ in registers,
//     W^T fragments from LDS -> dY_prev, ReLU-masked, stored; the previous layer's BatchNorm-backward sums) and ALSO
//     writes its dZ values, row-major, into an LDS exchange buffer: the first half of the output channels, barrier, the
//     second half, barrier (two buffers: while one half is being written the consumers read the other);
//   consumer q owns one 32 x 32 tile of dW per channel half -- (channel tile, input half) -- in persistent accumulators
//     (2 x 16 VGPRs) and adds dZ^T . relu(bn(z_prev)) of the quad's slabs to it: dZ^T fragments are 4-byte LDS reads of
//     the exchange buffer (lane = channel: conflict-free), the activation fragments are rebuilt from z_prev (L1 / L2 hits:
//     the producers read the same rows).  n_out = 64 has one tile per half and input half, so two consumers share a tile
//     and take two slabs each.
// The producers' global operands come through a ring of 8 steps (8 channels each) filled 7 steps ahead, across slab
// boundaries (one producer per SIMD: nothing else hides the HBM latency; a scheduling barrier per step keeps the compiler
// from sinking the loads to their uses), their per-row metadata a whole slab ahead, their LDS operands one step ahead.
// No dW traffic leaves the workgroup before its end: each consumer then stores its tiles into the workgroup's partial
// block(s); dw_reduce sums the blocks (f64).  A first version that had every wavefront do both products on its own slab
// and add 32 x 32 tiles into a dW block in LDS (ds_add_f32) ran at 365 us for layer 3: LDS float atomics retire ~1 lane
// per clock, and re-reading dZ in the accumulator layout cost another 130 us.
// ------------------------------------------------------------------------------------------------
template <int NJ, int GM>
__global__ __launch_bounds__(512, 2) void gemm_bwd_stream_kernel(DzSrc d, const int32_t* __restrict__ n_rows_dev, int n_rows_static,
                                                                  const float* __restrict__ W, DxEpi e, float* __restrict__ partial,
                                                                  unsigned long long* __restrict__ ts) {
    KTimer kt(ts);
    constexpr int NO = 8 * NJ, PW = NO + 4, NCH = NJ / 4, HCH = NCH / 2;    // chunks of 32 channels; per half
    constexpr int HC = NO / 2, HP = HC + 4;                                 // channels per half, exchange-buffer pitch
    constexpr int NCT = HC / 32;                                            // dW channel tiles per half (2 or 1)
    __shared__ __attribute__((aligned(16))) float Wt[64 * PW];
    __shared__ __attribute__((aligned(16))) float vec[3 * NO];          // P | Q | S
    __shared__ float red[2 * 4 * 64];
    __shared__ __attribute__((aligned(16))) float dzb[2 * 4 * 32 * HP];  // [half][slab of the quad][row][channel of the half]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    {   // W (n_out x 64, row-major) -> W^T in LDS
        constexpr int UW = NO * 16 / 512;
        float4 wr[UW];
#pragma unroll
        for (int it = 0; it < UW; ++it) wr[it] = ldg4(W + (size_t)(it * 512 + tid) * 4);
#pragma unroll
        for (int it = 0; it < UW; ++it) {
            const int u = it * 512 + tid;
            const int n = u >> 4, k4 = (u & 15) * 4;
            Wt[(k4 + 0) * PW + n] = wr[it].x; Wt[(k4 + 1) * PW + n] = wr[it].y;
            Wt[(k4 + 2) * PW + n] = wr[it].z; Wt[(k4 + 3) * PW + n] = wr[it].w;
        }
    }
    for (int i = tid; i < NO; i += 512) {
        float P, Q, S;
        dz_coef(d, i, P, Q, S, first_workgroup());
        vec[i] = P; vec[NO + i] = Q; vec[2 * NO + i] = S;
    }
    __syncthreads();
    const int n_slabs = (n_rows + 31) >> 5;
    const int n_quads = (n_slabs + 3) >> 2;
    const __amdgpu_buffer_rsrc_t zrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(e.zprev), 0, gad_nbytes(n_rows, 64 * 4), 0x00020000);   // rows past n_rows read as 0
    const int glane = (4 * half * 64 + l31) * 4;

    if (wave < 4) {
        // ---------------------------------------------------------------- producer: dX of slab 4 * quad + wave
        float ps[2], pt[2], pm[2], pi[2];
#pragma unroll
        for (int tk = 0; tk < 2; ++tk) {
            const int k = tk * 32 + l31;
            ps[tk] = e.ps[k]; pt[tk] = e.pt[k]; pm[tk] = e.pm[k]; pi[tk] = e.pi[k];
        }
        const __amdgpu_buffer_rsrc_t grsrc = __builtin_amdgcn_make_buffer_rsrc(e.gout, 0, gad_nbytes(n_rows, 64 * 4), 0x00020000);
        float sb[2] = {0.f, 0.f}, sg[2] = {0.f, 0.f};
        // operand ring: 8 steps of 8 output channels each (z, dY [, arg-max] of this lane's row: 16-byte loads), filled 7
        // steps ahead of their use and across slab boundaries -- with one producer per SIMD nothing else hides the HBM
        // latency of these loads (a two-chunk double buffer left ~2 us of stall per 32-channel chunk)
        constexpr int NU = NO / 8, RING = 8, AHEAD = RING - 1;
        float4 rz[RING], rg[RING];
        int4 ra[RING];
        auto row_of = [&](int sl) { return min(sl < n_slabs ? sl * 32 + l31 : 0, max(n_rows - 1, 0)); };
        auto load_u = [&](int r, int grp, int uu, int buf) {
            const unsigned n = 8 * uu + 4 * half;
            rz[buf] = ldg4(d.z + ((unsigned)r * NO + n));
            if (GM == 0) {
                rg[buf] = ldg4(d.G + ((unsigned)r * NO + n));
            } else {
                ra[buf] = *reinterpret_cast<const int4*>(d.argmax + ((unsigned)grp * NO + n));
                rg[buf] = ldg4(d.dout + ((unsigned)grp * NO + n));
            }
        };
        int quad = blockIdx.x;
        int slab = quad * 4 + wave;
        // row index / group / weight of this lane's row: fetched one slab (two for the group, which the ring's addresses
        // need mid-slab) before their use -- loads return in order, so waiting for a young load drains the whole ring
        int r_cur = row_of(slab), r_nxt = row_of(slab + 4 * gridDim.x);
        int grp_cur = GM == 1 ? d.row_grp[r_cur] : 0, grp_nxt = GM == 1 ? d.row_grp[r_nxt] : 0;
        float wrow = d.row_w ? d.row_w[r_cur] : 1.f;
#pragma unroll
        for (int i = 0; i < AHEAD; ++i) load_u(r_cur, grp_cur, i, i);
        float* const mybuf = dzb + (wave * 32 + l31) * HP + 4 * half;
        // LDS operands of a step (dZ coefficients of its 4 channels, W^T fragments): read one step ahead
        float4 P, Q, S, nb0, nb1;
        auto lds_operands = [&](int uu) {
            const int n = 8 * uu + 4 * half;
            P = *reinterpret_cast<const float4*>(vec + n);
            Q = *reinterpret_cast<const float4*>(vec + NO + n);
            S = *reinterpret_cast<const float4*>(vec + 2 * NO + n);
            nb0 = *reinterpret_cast<const float4*>(Wt + l31 * PW + n);
            nb1 = *reinterpret_cast<const float4*>(Wt + (32 + l31) * PW + n);
        };
        lds_operands(0);
        for (; quad < n_quads; quad += gridDim.x) {
            slab = quad * 4 + wave;
            const int r_nn = row_of(slab + 8 * gridDim.x);
            const int grp_nn = GM == 1 ? d.row_grp[r_nn] : 0;
            const float w_nxt = d.row_w ? d.row_w[r_nxt] : 1.f;
            const bool row_live = slab * 32 + l31 < n_rows;
            f32x16 acc[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
            float zp[2][16];
            const int zrow = (slab < n_slabs ? slab : 0) * 32 * 64 * 4;     // (a slab past the end: nothing is kept of it)
#pragma unroll
            for (int uu = 0; uu < NU; ++uu) {
                if (uu + AHEAD < NU) load_u(r_cur, grp_cur, uu + AHEAD, (uu + AHEAD) % RING);
                else load_u(r_nxt, grp_nxt, uu + AHEAD - NU, (uu + AHEAD) % RING);
                if (uu == 0) {                                             // z_prev for the epilogue: a whole slab ahead of its use
#pragma unroll
                    for (int v = 0; v < 16; ++v)
#pragma unroll
                        for (int t = 0; t < 2; ++t)
                            zp[t][v] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                                zrsrc, glane + t * 128, zrow + ((v & 3) + 8 * (v >> 2)) * 256, 0));
                }
                __builtin_amdgcn_sched_barrier(0);                         // (the scheduler would sink the loads to their uses)
                float* const hb = mybuf + (uu / (NU / 2)) * (4 * 32 * HP) + (uu % (NU / 2)) * 8;
                {
                    const float4 z = rz[uu % RING];
                    float4 g = rg[uu % RING];
                    if (GM == 1) {
                        const int4 a = ra[uu % RING];
                        const int rr = slab * 32 + l31;
                        g.x = a.x == rr ? g.x : 0.f; g.y = a.y == rr ? g.y : 0.f;
                        g.z = a.z == rr ? g.z : 0.f; g.w = a.w == rr ? g.w : 0.f;
                    }
                    float4 a4;
                    a4.x = P.x * g.x - wrow * fmaf(S.x, z.x, Q.x); a4.y = P.y * g.y - wrow * fmaf(S.y, z.y, Q.y);
                    a4.z = P.z * g.z - wrow * fmaf(S.z, z.z, Q.z); a4.w = P.w * g.w - wrow * fmaf(S.w, z.w, Q.w);
                    if (!row_live) a4 = make_float4(0.f, 0.f, 0.f, 0.f);          // rows past the end add nothing to dW
                    *reinterpret_cast<float4*>(hb) = a4;
                    const float4 b0 = nb0, b1 = nb1;
                    lds_operands((uu + 1) % NU);                           // the next step's, in flight under this step's MFMAs
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b0.x, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b1.x, acc[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b0.y, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b1.y, acc[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b0.z, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b1.z, acc[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b0.w, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b1.w, acc[1], 0, 0, 0);
                }
                if ((uu + 1) % (NU / 2) == 0) __syncthreads();             // this half of the quad's dZ is in the buffer
            }
            // epilogue: dY of the previous layer (ReLU-masked) + its BatchNorm-backward sums (the consumers are at work
            // on the second half meanwhile)
            const bool full = slab * 32 + 32 <= n_rows;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = acc_row(v, half);
                const bool live = slab * 32 + row < n_rows;
                const int rb = zrow + ((v & 3) + 8 * (v >> 2)) * 256;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const float gv = acc[t][v];
                    const float zv = zp[t][v];
                    const bool act = fmaf(zv, ps[t], pt[t]) > 0.f && live;
                    const float ga = act ? gv : 0.f;
                    if (full) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ga), grsrc, glane + t * 128, rb, GAD_STREAM_STORE_AUX);
                    else if (live) e.gout[(size_t)(slab * 32 + row) * 64 + t * 32 + l31] = ga;
                    sb[t] += ga;
                    sg[t] = fmaf(ga, (zv - pm[t]) * pi[t], sg[t]);
                }
            }
            r_cur = r_nxt; r_nxt = r_nn;
            grp_cur = grp_nxt; grp_nxt = grp_nn;
            wrow = w_nxt;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float s0 = sb[t] + __shfl_xor(sb[t], 32, 64);
            const float s1 = sg[t] + __shfl_xor(sg[t], 32, 64);
            if (lane < 32) { red[wave * 64 + t * 32 + lane] = s0; red[(4 + wave) * 64 + t * 32 + lane] = s1; }
        }
    } else {
        // ---------------------------------------------------------------- consumer: dW tiles (channel tile, input half b)
        const int q = wave - 4;
        const int b = q & 1;
        const int tcl = NCT == 2 ? (q >> 1) : 0;                            // channel tile within the half
        const int s0 = NCT == 2 ? 0 : 2 * (q >> 1);                         // slabs of the quad this wavefront takes
        constexpr int NS = NCT == 2 ? 4 : 2;
        const float psb = e.ps[32 * b + l31], ptb = e.pt[32 * b + l31];
        f32x16 aw[2];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int v = 0; v < 16; ++v) aw[h][v] = 0.f;
        // relu(bn(z_prev)) of the quad's slabs in the accumulator layout, kept for both channel halves; the next quad's
        // rows are requested as soon as the second half has used a slab's values (a whole exchange phase ahead)
        float yq[NS][16];
        auto load_y = [&](int slab, int s) {
            const int zrow = (slab < n_slabs ? slab : 0) * 32 * 64 * 4;     // (past the end: the producers wrote dZ = 0)
#pragma unroll
            for (int v = 0; v < 16; ++v)
                yq[s][v] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(zrsrc, glane + b * 128, zrow + ((v & 3) + 8 * (v >> 2)) * 256, 0));
        };
        const float* const rbase = dzb + (4 * half) * HP + 32 * tcl + l31;
#pragma unroll
        for (int s = 0; s < NS; ++s) load_y(blockIdx.x * 4 + s0 + s, s);
        for (int quad = blockIdx.x; quad < n_quads; quad += gridDim.x) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                __syncthreads();                                            // half h of this quad is in buffer h
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const float* rb = rbase + (h * 4 + s0 + s) * (32 * HP);
                    float dz[16];
#pragma unroll
                    for (int v = 0; v < 16; ++v) dz[v] = rb[((v & 3) + 8 * (v >> 2)) * HP];
                    if (h == 0) {
#pragma unroll
                        for (int v = 0; v < 16; ++v) yq[s][v] = fmaxf(fmaf(yq[s][v], psb, ptb), 0.f);
                    }
#pragma unroll
                    for (int v = 0; v < 16; ++v) aw[h] = __builtin_amdgcn_mfma_f32_32x32x2f32(dz[v], yq[s][v], aw[h], 0, 0, 0);
                    if (h == 1) load_y((quad + gridDim.x) * 4 + s0 + s, s);
                }
            }
        }
        // the workgroup's partial dW block(s): n_out = 64 -> two consumers share a tile, each writes its own block
        float* pout = partial + (size_t)(NCT == 2 ? blockIdx.x : 2 * blockIdx.x + (q >> 1)) * NO * 64;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int v = 0; v < 16; ++v) pout[(32 * (NCT * h + tcl) + acc_row(v, half)) * 64 + 32 * b + l31] = aw[h][v];
    }
    __syncthreads();
    if (tid < 64) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) { s0 += red[w * 64 + tid]; s1 += red[(4 + w) * 64 + tid]; }
        const int rep = blockIdx.x % GAD_STAT_REPLICAS;
        atomic_add_f64(e.dbeta + (size_t)rep * e.stat_stride + tid, (double)s0);
        atomic_add_f64(e.dgamma + (size_t)rep * e.stat_stride + tid, (double)s1);
    }
}

// ------------------------------------------------------------------------------------------------
// Split-bf16 form of the SA1 streaming backward (option "mfma_split": GAD_SPLIT_BWD_STREAM): gemm_bwd_stream_kernel (DW: dX and dW
// of one layer from one pass, 4 producer + 4 consumer wavefronts) and gemm_dx_stream_kernel (!DW: eight producers, no exchange).
//   producer: a lane owns row l31 of its slab and, per k16-step s, the 8 output channels 16 s + 8 half .. + 7 (two 16-byte
//     loads of z and dY through the operand ring); dZ = P*dY - w*(Q + S*z) is split into hi / mid / lo in registers -- the A
//     operand of six v_mfma_f32_32x32x16_bf16 per 32-column tile of dX against the TRANSPOSED weight mirror (LDS: three planes
//     [k][n_out (+ 8 pad)] copied from gad_split_weights' output, whose odd 16-blocks of n are stored negated: odd steps
//     accumulate into a second accumulator pair).  DW: the same hi / mid / lo registers go to the consumers TRANSPOSED: the two
//     lanes of a row pair exchange halves (DPP quad_perm + v_perm_b32) so that each holds {row 2j, row 2j + 1} of four of the
//     eight channels, and store 4 bytes per channel and plane into the exchange buffer [half][plane][slab][channel][32 rows]
//     (64-byte rows, 16-byte chunks XOR-swizzled by (channel >> 2) & 3: conflict-free ds_write_b32 and ds_read_b128).
//   consumer: dW tile (32 channels x 32 inputs) += dZ^T . y over the quad's slabs: A fragments = three ds_read_b128 of 8
//     consecutive rows of its channel, B fragments = relu(bn(z_prev)) of rows 16 st + 8 half .. + 7 loaded straight from
//     global memory (one value per lane and row, as the f32 kernel does), split once per slab and kept for both channel
//     halves; the rows 16 .. 31 of every slab carry NEGATED y and accumulate into a second accumulator pair.
// Results, partial-block layout, barrier structure and the epilogue are those of the f32 kernels.
// ------------------------------------------------------------------------------------------------
template <int NJ, int GM, bool DW>
__global__ __launch_bounds__(512, 2) void gemm_bwd_stream_split_kernel(DzSrc d, const int32_t* __restrict__ n_rows_dev, int n_rows_static,
                                                                        const uint16_t* __restrict__ wsp, int wsp_plane, DxEpi e,
                                                                        float* __restrict__ partial, unsigned long long* __restrict__ ts) {
    KTimer kt(ts);
    constexpr int NO = 8 * NJ, NS = NO / 16;                                // output channels, k16-steps
    constexpr int HC = NO / 2, NCT = HC / 32;                               // channels per exchange half, dW channel tiles per half
    constexpr int RB = 2 * NO + 16, WPL = 64 * RB;                          // bytes: mirror row in LDS (+ 16 pad), one plane
    constexpr int XSL = HC * 64, XPL = 4 * XSL, XBUF = 3 * XPL;             // bytes: exchange slab, plane (4 slabs), buffer (3 planes)
    __shared__ __attribute__((aligned(16))) unsigned char WtS[3 * WPL];
    __shared__ __attribute__((aligned(16))) float vec[3 * NO];              // P | Q | S
    __shared__ float red[2 * 8 * 64];
    __shared__ __attribute__((aligned(16))) unsigned char dzb[DW ? 2 * XBUF : 16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    {   // transposed weight mirror (3 planes x 64 rows x NO bf16, row pitch NO) -> LDS rows of RB bytes
        constexpr int CPR = NO / 8, UNITS = 3 * 64 * CPR, UW = (UNITS + 511) / 512;      // 16-byte chunks
        gad_u32x4 wr[UW];
#pragma unroll
        for (int it = 0; it < UW; ++it) {
            const int u = it * 512 + tid, uc = u < UNITS ? u : 0;
            const int pl = uc / (64 * CPR), rem = uc % (64 * CPR);
            wr[it] = *reinterpret_cast<const gad_u32x4*>(wsp + (size_t)pl * wsp_plane + (size_t)rem * 8);
        }
#pragma unroll
        for (int it = 0; it < UW; ++it) {
            const int u = it * 512 + tid;
            const int pl = u / (64 * CPR), rem = u % (64 * CPR), k = rem / CPR, c = rem % CPR;
            if (u < UNITS) *reinterpret_cast<gad_u32x4*>(WtS + pl * WPL + k * RB + c * 16) = wr[it];
        }
    }
    for (int i = tid; i < NO; i += 512) {
        float P, Q, S;
        dz_coef(d, i, P, Q, S, first_workgroup());
        vec[i] = P; vec[NO + i] = Q; vec[2 * NO + i] = S;
    }
    __syncthreads();
    const int n_slabs = (n_rows + 31) >> 5;
    const int n_quads = (n_slabs + 3) >> 2;
    const __amdgpu_buffer_rsrc_t zrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(e.zprev), 0, gad_nbytes(n_rows, 64 * 4), 0x00020000);   // rows past n_rows read as 0
    const int glane = (4 * half * 64 + l31) * 4;
    const int nprod = DW ? 4 : 8;                                           // producer wavefronts per workgroup

    if (!DW || wave < 4) {
        // ---------------------------------------------------------------- producer: dX of one slab per round
        float ps[2], pt[2], pm[2], pi[2];
#pragma unroll
        for (int tk = 0; tk < 2; ++tk) {
            const int k = tk * 32 + l31;
            ps[tk] = e.ps[k]; pt[tk] = e.pt[k]; pm[tk] = e.pm[k]; pi[tk] = e.pi[k];
        }
        const __amdgpu_buffer_rsrc_t grsrc = __builtin_amdgcn_make_buffer_rsrc(e.gout, 0, gad_nbytes(n_rows, 64 * 4), 0x00020000);
        float sb[2] = {0.f, 0.f}, sg[2] = {0.f, 0.f};
        // operand ring: entries of 4 channels (z, dY [, arg-max]: 16-byte loads); entry uu covers channels
        // 16 (uu >> 1) + 8 half + 4 (uu & 1) .. + 3, so a k16-step consumes an even / odd pair; filled AHEAD entries ahead, across slabs
        // The pooled source (GM = 1) reads its gradient / arg-max pair per GROUP (~26 consecutive rows share one: L1 / L2 hits), so that
        // pair rides a short ring of its own (RINGG = 4, one step ahead) -- with it in the long ring the kernel spilled.
        constexpr int NU = NO / 8, RING = 8, AHEAD = 6, RINGG = GM == 1 ? 4 : RING, AHEADG = GM == 1 ? 2 : AHEAD;
        static_assert(NU % RING == 0 && NU % RINGG == 0, "a slab's entries must fill the rings a whole number of times");
        float4 rz[RING], rg[RINGG];
        int4 ra[RINGG];
        auto row_of = [&](int sl) { return min(sl < n_slabs ? sl * 32 + l31 : 0, max(n_rows - 1, 0)); };
        auto load_z = [&](int r, int uu) {
            const unsigned n = 16 * (uu >> 1) + 8 * half + 4 * (uu & 1);
            rz[uu % RING] = ldg4(d.z + ((unsigned)r * NO + n));
            if (GM == 0) rg[uu % RINGG] = ldg4(d.G + ((unsigned)r * NO + n));
        };
        auto load_g = [&](int grp, int uu) {              // (GM = 1)
            const unsigned n = 16 * (uu >> 1) + 8 * half + 4 * (uu & 1);
            ra[uu % RINGG] = *reinterpret_cast<const int4*>(d.argmax + ((unsigned)grp * NO + n));
            rg[uu % RINGG] = ldg4(d.dout + ((unsigned)grp * NO + n));
        };
        // slabs: DW: quad q = blockIdx.x + i * gridDim.x, slab 4 q + wave; !DW: the wave-major dealing of gemm_dx_stream_kernel
        const int round_stride = DW ? 4 * gridDim.x : 8 * gridDim.x;
        int slab = DW ? blockIdx.x * 4 + wave : wave * gridDim.x + blockIdx.x;
        const int slab_limit = DW ? n_quads * 4 : n_slabs;
        int r_cur = row_of(slab), r_nxt = row_of(slab + round_stride);
        int grp_cur = GM == 1 ? d.row_grp[r_cur] : 0, grp_nxt = GM == 1 ? d.row_grp[r_nxt] : 0;
        float wrow = d.row_w ? d.row_w[r_cur] : 1.f;
#pragma unroll
        for (int i = 0; i < AHEAD; ++i) load_z(r_cur, i);
        if (GM == 1) {
#pragma unroll
            for (int i = 0; i < AHEADG; ++i) load_g(grp_cur, i);
        }
        // exchange store position of this lane: row pair l31 >> 1 (4 bytes) of channel (c0 & (HC - 1)) + 2 i + (l31 & 1)
        const unsigned psel = (l31 & 1) ? 0x03020706u : 0x05040100u;        // v_perm_b32 selector: {even row | odd row} of the lane's channels
        const unsigned rsg = (l31 & 1) ? 0x80000000u : 0u;                  // sign of this lane's row in the products (header of the split section)
        const int xq = l31 >> 3, xin = ((l31 >> 1) & 3) * 4;                // 16-byte chunk (before the swizzle), byte inside it
        const unsigned char* const wb = WtS + l31 * RB + 16 * half;
        for (; slab < slab_limit; slab += round_stride) {
            const int r_nn = row_of(slab + 2 * round_stride);
            const int grp_nn = GM == 1 ? d.row_grp[r_nn] : 0;
            const float w_nxt = d.row_w ? d.row_w[r_nxt] : 1.f;
            const bool row_live = slab * 32 + l31 < n_rows;
            f32x16 acc[2], an[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) { acc[t][v] = 0.f; an[t][v] = 0.f; }
            float zp[2][16];
            const int zrow = (slab < n_slabs ? slab : 0) * 32 * 64 * 4;     // (a slab past the end: nothing is kept of it)
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2) {
#pragma unroll
                for (int ee = 0; ee < 2; ++ee) {
                    const int uu = 2 * s2 + ee + AHEAD;
                    if (uu < NU) load_z(r_cur, uu); else load_z(r_nxt, uu - NU);
                    if (GM == 1) {
                        const int ug = 2 * s2 + ee + AHEADG;
                        if (ug < NU) load_g(grp_cur, ug); else load_g(grp_nxt, ug - NU);
                    }
                }
                if (s2 == 0) {                                              // z_prev for the epilogue: a whole slab ahead of its use
#pragma unroll
                    for (int v = 0; v < 16; ++v)
#pragma unroll
                        for (int t = 0; t < 2; ++t)
                            zp[t][v] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                                zrsrc, glane + t * 128, zrow + ((v & 3) + 8 * (v >> 2)) * 256, 0));
                }
                __builtin_amdgcn_sched_barrier(0);                          // (the scheduler would sink the loads to their uses)
                // B fragments of this step (transposed mirror rows l31, 32 + l31; channels 16 s + 8 half .. + 7)
                gad_u32x4 BH[2], BM[2], BL[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const unsigned char* q = wb + t * (32 * RB) + 32 * s2;
                    BH[t] = *reinterpret_cast<const gad_u32x4*>(q);
                    BM[t] = *reinterpret_cast<const gad_u32x4*>(q + WPL);
                    BL[t] = *reinterpret_cast<const gad_u32x4*>(q + 2 * WPL);
                }
                unsigned ah[4], am[4], al[4];
#pragma unroll
                for (int ee = 0; ee < 2; ++ee) {
                    const int uu = 2 * s2 + ee;
                    const int n = 16 * s2 + 8 * half + 4 * ee;
                    const float4 P = *reinterpret_cast<const float4*>(vec + n);
                    const float4 Q = *reinterpret_cast<const float4*>(vec + NO + n);
                    const float4 S = *reinterpret_cast<const float4*>(vec + 2 * NO + n);
                    const float4 z = rz[uu % RING];
                    float4 g = rg[uu % RINGG];
                    if (GM == 1) {
                        const int4 a = ra[uu % RINGG];
                        const int rr = slab * 32 + l31;
                        g.x = a.x == rr ? g.x : 0.f; g.y = a.y == rr ? g.y : 0.f;
                        g.z = a.z == rr ? g.z : 0.f; g.w = a.w == rr ? g.w : 0.f;
                    }
                    float4 a4;
                    a4.x = P.x * g.x - wrow * fmaf(S.x, z.x, Q.x); a4.y = P.y * g.y - wrow * fmaf(S.y, z.y, Q.y);
                    a4.z = P.z * g.z - wrow * fmaf(S.z, z.z, Q.z); a4.w = P.w * g.w - wrow * fmaf(S.w, z.w, Q.w);
                    if (!row_live) a4 = make_float4(0.f, 0.f, 0.f, 0.f);       // rows past the end add nothing to dW
                    // (odd rows enter negated -- here and, through the exchange, in the consumers, which negate y of odd rows)
                    gad_split2(__uint_as_float(__float_as_uint(a4.x) ^ rsg), __uint_as_float(__float_as_uint(a4.y) ^ rsg), ah[2 * ee], am[2 * ee], al[2 * ee]);
                    gad_split2(__uint_as_float(__float_as_uint(a4.z) ^ rsg), __uint_as_float(__float_as_uint(a4.w) ^ rsg), ah[2 * ee + 1], am[2 * ee + 1], al[2 * ee + 1]);
                }
                const gad_u32x4 AH = {ah[0], ah[1], ah[2], ah[3]}, AM = {am[0], am[1], am[2], am[3]}, AL = {al[0], al[1], al[2], al[3]};
                if (DW) {
                    // transposed hand-over: channel cl = (16 s + 8 half) % HC + 2 i + (l31 & 1), rows {l31 & ~1, l31 | 1}
                    unsigned char* hb = dzb + (s2 / (NS / 2)) * XBUF + wave * XSL + xin;
                    const int cbase = (16 * s2 + 8 * half) % HC + (l31 & 1);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int cl = cbase + 2 * i;
                        unsigned char* q = hb + cl * 64 + ((xq ^ ((cl >> 2) & 3)) << 4);
                        const unsigned own[3] = {ah[i], am[i], al[i]};
#pragma unroll
                        for (int pl = 0; pl < 3; ++pl) {
                            const unsigned nbr = (unsigned)__builtin_amdgcn_update_dpp(0, (int)own[pl], 0xB1, 0xf, 0xf, false);   // lane ^ 1
                            *reinterpret_cast<unsigned*>(q + pl * XPL) = __builtin_amdgcn_perm(nbr, own[pl], psel);
                        }
                    }
                }
                // the six products of weight >= 2^-16, smallest first; odd steps (negated mirror values) -> the second pair
#define GAD_SPB(A, B)                                                                                                          \
                _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                                                \
                    if (s2 & 1) an[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gad_as_bf16x8(A), gad_as_bf16x8(B[t]), an[t], 0, 0, 0);   \
                    else acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gad_as_bf16x8(A), gad_as_bf16x8(B[t]), acc[t], 0, 0, 0); \
                }
                GAD_SPB(AL, BH) GAD_SPB(AH, BL) GAD_SPB(AM, BM) GAD_SPB(AM, BH) GAD_SPB(AH, BM) GAD_SPB(AH, BH)
#undef GAD_SPB
                if (DW && (s2 + 1) % (NS / 2) == 0) __syncthreads();        // this half of the quad's dZ is in the buffer
            }
            // epilogue: dY of the previous layer (ReLU-masked) + its BatchNorm-backward sums
            const bool full = slab * 32 + 32 <= n_rows;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = acc_row(v, half);
                const bool live = slab * 32 + row < n_rows;
                const int rb = zrow + ((v & 3) + 8 * (v >> 2)) * 256;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const float gv = (v & 1) ? an[t][v] - acc[t][v] : acc[t][v] - an[t][v];
                    const float zv = live ? zp[t][v] : 0.f;
                    const bool act = fmaf(zv, ps[t], pt[t]) > 0.f && live;
                    const float ga = act ? gv : 0.f;
                    if (full) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ga), grsrc, glane + t * 128, rb, GAD_STREAM_STORE_AUX);
                    else if (live) e.gout[(size_t)(slab * 32 + row) * 64 + t * 32 + l31] = ga;
                    sb[t] += ga;
                    sg[t] = fmaf(ga, (zv - pm[t]) * pi[t], sg[t]);
                }
            }
            r_cur = r_nxt; r_nxt = r_nn;
            grp_cur = grp_nxt; grp_nxt = grp_nn;
            wrow = w_nxt;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float s0 = sb[t] + __shfl_xor(sb[t], 32, 64);
            const float s1 = sg[t] + __shfl_xor(sg[t], 32, 64);
            if (lane < 32) { red[wave * 64 + t * 32 + lane] = s0; red[(8 + wave) * 64 + t * 32 + lane] = s1; }
        }
    } else {
        // ---------------------------------------------------------------- consumer: dW tiles (channel tile, input half b)
        const int q = wave - 4;
        const int b = q & 1;
        const int tcl = NCT == 2 ? (q >> 1) : 0;                            // channel tile within the half
        const int s0 = NCT == 2 ? 0 : 2 * (q >> 1);                         // slabs of the quad this wavefront takes
        constexpr int NSC = NCT == 2 ? 4 : 2;
        const float psb = e.ps[32 * b + l31], ptb = e.pt[32 * b + l31];
        f32x16 aw[2], awn[2];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int v = 0; v < 16; ++v) { aw[h][v] = 0.f; awn[h][v] = 0.f; }
        // z_prev of the quad's slabs: lane (input column 32 b + l31, half) holds rows 16 st + 8 half + i of a slab -- the B layout
        const int ylane = (8 * half * 64 + 32 * b + l31) * 4;
        float yr[NSC][16];
        gad_u32x4 YH[NSC][2], YM[NSC][2], YL[NSC][2];
        auto load_y = [&](int slab, int sl) {
            const int zrow = (slab < n_slabs ? slab : 0) * 32 * 64 * 4;     // (past the end: the producers wrote dZ = 0)
#pragma unroll
            for (int v = 0; v < 16; ++v)
                yr[sl][v] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(zrsrc, ylane, zrow + (16 * (v >> 3) + (v & 7)) * 256, 0));
        };
        const int cl = 32 * tcl + l31;
        const unsigned char* const rbase = dzb + cl * 64;
        const int fo = ((half ^ ((cl >> 2) & 3)) << 4);
#pragma unroll
        for (int sl = 0; sl < NSC; ++sl) load_y(blockIdx.x * 4 + s0 + sl, sl);
        for (int quad = blockIdx.x; quad < n_quads; quad += gridDim.x) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                __syncthreads();                                            // half h of this quad is in buffer h
#pragma unroll
                for (int sl = 0; sl < NSC; ++sl) {
                    if (h == 0) {                                           // relu(bn(z_prev)) -> hi / mid / lo, rows 16 .. 31 negated
#pragma unroll
                        for (int st = 0; st < 2; ++st) {
                            unsigned yh[4], ym[4], yl[4];
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                float y0 = fmaxf(fmaf(yr[sl][8 * st + 2 * i], psb, ptb), 0.f), y1 = fmaxf(fmaf(yr[sl][8 * st + 2 * i + 1], psb, ptb), 0.f);
                                // dZ of the odd rows arrives negated: undo it on y; rows 16 .. 31 are negated for the accumulator pair
                                if (st) y0 = -y0; else y1 = -y1;
                                gad_split2(y0, y1, yh[i], ym[i], yl[i]);
                            }
                            YH[sl][st] = gad_u32x4{yh[0], yh[1], yh[2], yh[3]};
                            YM[sl][st] = gad_u32x4{ym[0], ym[1], ym[2], ym[3]};
                            YL[sl][st] = gad_u32x4{yl[0], yl[1], yl[2], yl[3]};
                        }
                    }
                    const unsigned char* rb = rbase + h * XBUF + (s0 + sl) * XSL;
#pragma unroll
                    for (int st = 0; st < 2; ++st) {
                        const int off = fo ^ (st << 5);
                        const gad_u32x4 AH = *reinterpret_cast<const gad_u32x4*>(rb + off);
                        const gad_u32x4 AM = *reinterpret_cast<const gad_u32x4*>(rb + XPL + off);
                        const gad_u32x4 AL = *reinterpret_cast<const gad_u32x4*>(rb + 2 * XPL + off);
#define GAD_SPC(A, B)                                                                                                          \
                        if (st) awn[h] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gad_as_bf16x8(A), gad_as_bf16x8(B[sl][st]), awn[h], 0, 0, 0); \
                        else aw[h] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gad_as_bf16x8(A), gad_as_bf16x8(B[sl][st]), aw[h], 0, 0, 0);
                        GAD_SPC(AL, YH) GAD_SPC(AH, YL) GAD_SPC(AM, YM) GAD_SPC(AM, YH) GAD_SPC(AH, YM) GAD_SPC(AH, YH)
#undef GAD_SPC
                    }
                    if (h == 1) load_y((quad + gridDim.x) * 4 + s0 + sl, sl);
                }
            }
        }
        // the workgroup's partial dW block(s): n_out = 64 -> two consumers share a tile, each writes its own block
        float* pout = partial + (size_t)(NCT == 2 ? blockIdx.x : 2 * blockIdx.x + (q >> 1)) * NO * 64;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int v = 0; v < 16; ++v) pout[(32 * (NCT * h + tcl) + acc_row(v, half)) * 64 + 32 * b + l31] = aw[h][v] - awn[h][v];
    }
    __syncthreads();
    if (tid < 64) {
        float s0 = 0.f, s1 = 0.f;
        for (int w = 0; w < nprod; ++w) { s0 += red[w * 64 + tid]; s1 += red[(8 + w) * 64 + tid]; }
        const int rep = blockIdx.x % GAD_STAT_REPLICAS;
        atomic_add_f64(e.dbeta + (size_t)rep * e.stat_stride + tid, (double)s0);
        atomic_add_f64(e.dgamma + (size_t)rep * e.stat_stride + tid, (double)s1);
    }
}

bool dx_streamable(const gad_gemm_dx_args& a, bool vec) {
    if (g_opt.deterministic || !g_opt.dx_stream || !vec || a.n_groups != 1 || a.dz_off[0] != 0 || a.w_off[0] != 0 || a.gout_off[0] != 0) return false;
    if (a.n_rows < 32768 || a.epilogue != 0 || a.k_valid != 64 || a.Kp != 64 || a.gout_pitch != 64) return false;
    if (a.n_out[0] != 64 && a.n_out[0] != 128) return false;
    if (!a.prev_dbeta || a.zprev_pitch != 64 || !a.store_masked) return false;
    const gad_dz_src& d = a.dz;
    const bool coef = (d.coefP && d.coefQ && d.coefS);
    if (!d.z || d.z_pitch != a.n_out[0] || !d.scale || !d.relu || !d.premasked || !coef) return false;
    if (d.gmode == 0 ? d.g_pitch != a.n_out[0] : d.c != a.n_out[0]) return false;
    return (long long)a.n_rows * 128 * 4 <= (1ll << 31);
}

// gad_gemm_dx's streaming route (dx_streamable): the dX-only kernel, or the split form of the fused one with DW = false
int dx_stream_launch(const gad_gemm_dx_args* a, const DzSrc& d, const DxEpi& e, unsigned long long* ts, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int rows = a->n_rows;
    const int slabs = gad_cdiv(rows, 32);
    int gx = gad_cdiv(slabs, 8); if (gx > 256) gx = 256;
    if (split_on(GAD_SPLIT_BWD_STREAM) && a->W_split_t && a->W_split_t_pitch == a->n_out[0] && a->W_split_t_plane >= 64 * a->n_out[0]) {
#define LAUNCH_DXSS(NJ, GM) hipLaunchKernelGGL((gemm_bwd_stream_split_kernel<NJ, GM, false>), dim3(gx), dim3(512), 0, st, d, a->n_rows_dev, rows, \
                                            a->W_split_t, a->W_split_t_plane, e, nullptr, ts)
        if (a->n_out[0] == 128) { if (a->dz.gmode == 0) LAUNCH_DXSS(16, 0); else LAUNCH_DXSS(16, 1); }
        else { if (a->dz.gmode == 0) LAUNCH_DXSS(8, 0); else LAUNCH_DXSS(8, 1); }
#undef LAUNCH_DXSS
        GAD_CHECK_LAUNCH("gemm_dx(stream split)");
        return GAD_OK;
    }
#define LAUNCH_DXS(NJ, GM) hipLaunchKernelGGL((gemm_dx_stream_kernel<NJ, GM>), dim3(gx), dim3(512), 0, st, d, a->n_rows_dev, rows, a->W, e, ts)
    if (a->n_out[0] == 128) { if (a->dz.gmode == 0) LAUNCH_DXS(16, 0); else LAUNCH_DXS(16, 1); }
    else { if (a->dz.gmode == 0) LAUNCH_DXS(8, 0); else LAUNCH_DXS(8, 1); }
#undef LAUNCH_DXS
    GAD_CHECK_LAUNCH("gemm_dx(stream)");
    return GAD_OK;
}

// ------------------------------------------------------------------------------------------------
// FUSED wide-tile backward for the MID-SIZE layers (SA2 / SA3; round 4): dX AND dW of one layer from ONE pass over dZ.
// The separate kernels (gemm_dx_wide / gemm_dw_wide) each form dZ = P*dY - w*(Q + S*z) from their own loads of z and dY
// (1 + K/128 times per element for dX, once per 128-wide k block for dW), and each launch is only a few K-tiles deep per
// workgroup: barrier and load latency, not MFMA issue, is what they spend their time on (0.17 - 0.25 of the FP32-MFMA peak
// inside the step).  Here a workgroup owns 64-row tiles x ONE 64-wide block of input channels (grid.y = K / 64) and walks the
// layer's N output channels in steps of 64: every staged dZ tile [64 rows x 64 channels] and W tile [64 channels x 64 k]
// feeds 32 dX MFMAs (32 rows x 32 k per wavefront, reduction over the 64 channels) AND 32 dW MFMAs (32 channels x 32 k per
// wavefront, reduction over the tile's 64 rows) -- twice the MFMA work per barrier, per staged byte and per dZ formation.
//   * dZ tile: row-major [row][64 + 4] -- the dX A fragments are ds_read_b128 along the channels (k = 8j+4h+i order), the dW
//     A fragments (dZ^T) are conflict-free ds_read_b32 across the channels of rows 2s + h;
//   * W tile as stored ([n][64 + 4]): the dX B fragments are ds_read_b32 across k of row n = 8j+4h+i -- no transposing store;
//   * the dW B operand -- the layer INPUT X[row][k], k = this lane's column -- never touches LDS: 32 coalesced 4-byte loads
//     per lane and row tile (relu(scale * z_prev + shift) with the lane's own scale / shift, or the gathered feature), held
//     in 32 registers and reused by every channel step of the tile;
//   * the dW accumulators (N / 64 per wavefront: the wavefront pair (w >> 1) splits each 64-channel step by halves) persist
//     over the workgroup's row tiles and leave as ONE partial block per workgroup; dw_reduce sums the blocks in f64.  (f64
//     atomics straight into the arena are SLOWER than slab + reduce on this part: 5.6 vs 3.5 us per million partial
//     elements, tools/ubench/atomic_reduce.hip -> profiles/r04_atomic_reduce.txt.)
//   * dX epilogue as in gemm_dx_wide: dY of the previous layer masked by its ReLU + that layer's BatchNorm-backward sums, or
//     (L1: the gathered first layers) float atomics into the points' feature gradients; L1 also forms the three coordinate
//     columns of dW with vector FMAs while dZ is staged (k block 0 only).
// One LDS buffer + register prefetch (two barriers per 64 MFMAs): 36 KB of LDS and <= 128 VGPRs of accumulators leave room
// for 3 - 4 workgroups per CU, which is what hides the barriers here.
// ------------------------------------------------------------------------------------------------
template <int NIT, int GM, int L1>
__global__ __launch_bounds__(256, NIT >= 8 ? 1 : 2) void gemm_bwd_wide_kernel(DzSrc d, XSrc x, const int32_t* __restrict__ n_rows_dev,
                                                               int n_rows_static, const float* __restrict__ W, int Kp, DxEpi e,
                                                               float* __restrict__ partial, unsigned long long* __restrict__ ts) {
    KTimer kt_(ts);
    constexpr int N = NIT * 64, P = 68, TILE = 64 * P;
    __shared__ __attribute__((aligned(16))) float smem[2 * TILE + 3 * N + 64 * 4];
    __shared__ int32_t ptS[64];
    float* As = smem;
    float* Ws = smem + TILE;
    float* vP = smem + 2 * TILE;                          // P | Q | S of the layer's N channels
    float* relS = vP + 3 * N;                             // L1: [row][4] = src_xyz[pt] - ctr_xyz[grp]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;              // dX: row half / k half;  dW: channel half of the step / k half
    const int l31 = lane & 31, half = lane >> 5;
    const int k0 = blockIdx.y * 64;
    const int n_rows = n_rows_dev ? min(*n_rows_dev, n_rows_static) : n_rows_static;
    const int n_tiles = (n_rows + 63) >> 6;
    const int c4 = (tid & 15) * 4, sr = tid >> 4;         // staging: 16-byte chunk of the 64-wide tile, rows sr + 16 u
    for (int i = tid; i < N; i += 256) {
        float Pc, Qc, Sc;
        dz_coef(d, i, Pc, Qc, Sc, first_workgroup());
        vP[i] = Pc; vP[N + i] = Qc; vP[2 * N + i] = Sc;
    }
    // every global operand goes through a buffer descriptor: 32-bit per-lane byte offsets (one VGPR each, set up once per
    // tile) + a wave-uniform scalar offset per access, instead of a 64-bit pointer pair per unrolled load
    const int gpitch = GM == 0 ? d.g_pitch : d.c;
    // z, dY and the layer input are bounded by the LIVE rows: a read past them returns 0, so a dead row's dZ is exactly 0
    // (its weight is 0 as well) without a select per element -- on this part every VALU instruction is MFMA issue time
    const __amdgpu_buffer_rsrc_t zr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.z), 0, gad_nbytes(n_rows, d.z_pitch * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t gr_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(GM == 0 ? d.G : d.dout), 0,
                                                                         GM == 0 ? gad_nbytes(n_rows, gpitch * 4) : GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(GM == 0 ? d.row_grp : d.argmax), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W), 0, GAD_BUF_MAX, 0x00020000);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(L1 ? x.feat : x.zin), 0,
                                                                        L1 ? GAD_BUF_MAX : gad_nbytes(n_rows, x.zin_pitch * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t sr_ = __builtin_amdgcn_make_buffer_rsrc(partial, 0, GAD_BUF_MAX, 0x00020000);
    // previous layer's raw output / the gradient this launch writes: bounded by the live rows (reads past them give 0,
    // stores past them are dropped)
    const int zp_pitch4 = L1 ? 0 : e.zprev_pitch * 4, go_pitch4 = L1 ? 0 : e.gout_pitch * 4;
    const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(L1 ? W : e.zprev), 0, L1 ? 0 : gad_nbytes(n_rows, zp_pitch4), 0x00020000);
    const __amdgpu_buffer_rsrc_t or_ = __builtin_amdgcn_make_buffer_rsrc(L1 ? const_cast<float*>(W) : e.gout, 0, L1 ? 0 : gad_nbytes(n_rows, go_pitch4), 0x00020000);
    const int kx = k0 + wn * 32 + l31;                    // this lane's input channel (dW column, dX column)
    float xs = 1.f, xt = 0.f, ps = 0.f, pt = 0.f, pm = 0.f, pi = 0.f;
    if (!L1) { xs = x.scale[kx]; xt = x.shift[kx]; ps = e.ps[kx]; pt = e.pt[kx]; pm = e.pm[kx]; pi = e.pi[kx]; }
    const bool coords = L1 && k0 == 0;
    float wx[NIT][3];                                     // coords: channel it * 64 + lane, rows wave * 16 .. + 15 of every tile
    if (L1) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) { wx[it][0] = 0.f; wx[it][1] = 0.f; wx[it][2] = 0.f; }
    }
    f32x16 accw[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it)
#pragma unroll
        for (int v = 0; v < 16; ++v) accw[it][v] = 0.f;
    float cb = 0.f, cg = 0.f;
    int vw[4];                                            // W staging offsets: rows sr + 16 u of the step's 64 channels
#pragma unroll
    for (int u = 0; u < 4; ++u) vw[u] = ((sr + 16 * u) * Kp + k0 + c4) * 4;
    const int xpitch4 = L1 ? x.feat_c * 4 : x.zin_pitch * 4;
    const int vx = (half * (L1 ? 0 : x.zin_pitch) + kx) * 4;             // X fragment lane offset (row 2 s + half, column kx)
    const int vzp = (4 * half * (L1 ? 0 : e.zprev_pitch) + kx) * 4, vgo = (4 * half * (L1 ? 0 : e.gout_pitch) + kx) * 4;
    // this thread's four staged rows of a tile (offsets, weights) and the staging registers; the NEXT tile's first step is
    // loaded under the current tile's last MFMAs and epilogue (cross-tile prefetch: a workgroup has 1 - 3 tiles, so the
    // staging latency in front of every tile was a third of its time)
    int vz[4], vg[4];
    unsigned rtrue[4];                                    // GM = 1: the row an arg-max must name; a row past the live rows matches none
    float wrow[4];
    float4 rz[4], rg[4], rb[4];
    gad_u32x4 ra[4];
    auto meta = [&](int row0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = row0 + sr + 16 * u;
            const bool live = r < n_rows;
            const int rr = live ? r : max(n_rows - 1, 0);
            const float w = d.row_w ? d.row_w[rr] : 1.f;
            wrow[u] = live ? w : 0.f;
            rtrue[u] = live ? (unsigned)r : 0xffffffffu;
            vz[u] = (r * d.z_pitch + c4) * 4;             // (the true row: past the live rows the bounded descriptor reads 0)
            vg[u] = ((GM == 1 ? d.row_grp[rr] : r) * gpitch + c4) * 4;
        }
    };
    auto load_regs = [&](int it) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            rz[u] = buf_ld4(zr, vz[u], it * 256);
            rg[u] = buf_ld4(gr_, vg[u], it * 256);
            if (GM == 1) ra[u] = __builtin_amdgcn_raw_buffer_load_b128(ar, vg[u], it * 256, 0);
            rb[u] = buf_ld4(wr, vw[u], it * 256 * Kp);
        }
    };
    if ((int)blockIdx.x < n_tiles) { meta(blockIdx.x << 6); load_regs(0); }
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int row0 = tile << 6;
        __syncthreads();                                  // vP visible; the previous tile's LDS reads (As, Ws, ptS, relS) are done
        if (L1 && tid < 64) {
            const int r = min(row0 + tid, max(n_rows - 1, 0));
            const int p = x.row_pt[r];
            ptS[tid] = p;
            const float* q = x.src_xyz + (size_t)p * 3;
            float q0 = q[0], q1 = q[1], q2 = q[2];
            if (x.ctr_xyz) {
                const float* cp = x.ctr_xyz + (size_t)x.row_grp[r] * 3;
                q0 = __fsub_rn(q0, cp[0]); q1 = __fsub_rn(q1, cp[1]); q2 = __fsub_rn(q2, cp[2]);
            }
            *reinterpret_cast<float4*>(relS + 4 * tid) = make_float4(q0, q1, q2, 0.f);
        }
        if (L1) __syncthreads();
        // ---- the dW B operand: X[row0 + 2 s + half][kx], s = 0 .. 31, straight into registers (activated below)
        float xf[32];
#pragma unroll
        for (int sidx = 0; sidx < 32; ++sidx) {
            if (L1) {
                xf[sidx] = buf_ld(xr, ptS[2 * sidx + half] * xpitch4 + vx, 0);
            } else {
                xf[sidx] = buf_ld(xr, vx, (row0 + 2 * sidx) * xpitch4);     // (past the live rows: 0; their dZ is 0 as well)
            }
        }
        f32x16 accx;
#pragma unroll
        for (int v = 0; v < 16; ++v) accx[v] = 0.f;
        float zp[16];
        const int rb0 = row0 + wm * 32;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (it > 0) __syncthreads();                  // the previous step's fragment reads are done
            {   // registers -> LDS: dZ formed once per staged element
                const int nb = it * 64 + c4;
                const float4 P4 = *reinterpret_cast<const float4*>(vP + nb), Q4 = *reinterpret_cast<const float4*>(vP + N + nb);
                const float4 S4 = *reinterpret_cast<const float4*>(vP + 2 * N + nb);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float4 g = rg[u];
                    const float4 z = rz[u];
                    if (GM == 1) {
                        // the true row, not the clamped one; a dead row takes no gradient even where the group's arg-max names it
                        // (its dZ must be exactly 0: the statistics and dW below count on it), as in the separate kernels
                        const unsigned r = rtrue[u];
                        g.x = ra[u].x == r ? g.x : 0.f; g.y = ra[u].y == r ? g.y : 0.f;
                        g.z = ra[u].z == r ? g.z : 0.f; g.w = ra[u].w == r ? g.w : 0.f;
                    }
                    const float w = wrow[u];
                    float4 v;
                    v.x = P4.x * g.x - w * fmaf(S4.x, z.x, Q4.x); v.y = P4.y * g.y - w * fmaf(S4.y, z.y, Q4.y);
                    v.z = P4.z * g.z - w * fmaf(S4.z, z.z, Q4.z); v.w = P4.w * g.w - w * fmaf(S4.w, z.w, Q4.w);
                    *reinterpret_cast<float4*>(As + (sr + 16 * u) * P + c4) = v;
                    *reinterpret_cast<float4*>(Ws + (sr + 16 * u) * P + c4) = rb[u];
                }
            }
            if (it + 1 < NIT) {
                load_regs(it + 1);
            } else {
                const int nxt = tile + gridDim.x;         // next tile's first step (wave-uniform branch)
                if (nxt < n_tiles) { meta(nxt << 6); load_regs(0); }
                if (!L1) {                                // this tile's z_prev for the epilogue: in flight under the last MFMAs
#pragma unroll
                    for (int v = 0; v < 16; ++v) zp[v] = buf_ld(pr, vzp, (rb0 + (v & 3) + 8 * (v >> 2)) * zp_pitch4);
                }
            }
            if (it == 0) {                                // activate the X fragments once per tile (their loads have had a whole staging pass)
                if (!L1) {
#pragma unroll
                    for (int sidx = 0; sidx < 32; ++sidx) xf[sidx] = fmaxf(fmaf(xf[sidx], xs, xt), 0.f);
                }
            }
            __syncthreads();
            if (coords) {                                 // dW[n][feat_c .. + 2] += dZ[r][n] * rel[r][0 .. 2]: lane = channel, 16 rows per wavefront
                const float* ap = As + (wave * 16) * P + lane;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float a = ap[r * P];
                    const float4 q = *reinterpret_cast<const float4*>(relS + 4 * (wave * 16 + r));
                    wx[it][0] = fmaf(a, q.x, wx[it][0]); wx[it][1] = fmaf(a, q.y, wx[it][1]); wx[it][2] = fmaf(a, q.z, wx[it][2]);
                }
            }
            // ---- dX: 32 rows x 32 k of this wavefront, reduction over the step's 64 channels
            {
                const float* ap = As + (wm * 32 + l31) * P + 4 * half;
                const float* bp = Ws + (4 * half) * P + wn * 32 + l31;
                float4 a4 = *reinterpret_cast<const float4*>(ap);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float4 an = a4;
                    if (j + 1 < 8) an = *reinterpret_cast<const float4*>(ap + 8 * (j + 1));
                    const float b0 = bp[(8 * j + 0) * P], b1 = bp[(8 * j + 1) * P], b2 = bp[(8 * j + 2) * P], b3 = bp[(8 * j + 3) * P];
                    accx = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b0, accx, 0, 0, 0);
                    accx = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b1, accx, 0, 0, 0);
                    accx = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b2, accx, 0, 0, 0);
                    accx = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b3, accx, 0, 0, 0);
                    a4 = an;
                }
            }
            // ---- dW: 32 channels (half wm of the step) x 32 k, reduction over the tile's 64 rows
            {
                const float* ap = As + half * P + wm * 32 + l31;
#pragma unroll
                for (int s8 = 0; s8 < 4; ++s8) {
                    float a[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) a[q] = ap[(2 * (8 * s8 + q)) * P];
#pragma unroll
                    for (int q = 0; q < 8; ++q) accw[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], xf[8 * s8 + q], accw[it], 0, 0, 0);
                }
            }
        }
        // ---- dX epilogue
        if (L1) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int il = wm * 32 + acc_row(v, half);
                if (row0 + il < n_rows) atomic_add_f32(e.dfeat + (size_t)ptS[il] * e.feat_c + kx, accx[v]);
            }
        } else {
            // (a row past the live count: z_prev reads 0, its accumulator row is exactly 0 -- dZ = 0 -- and the store is dropped)
            const float npm = -pm * pi;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float ga = fmaf(zp[v], ps, pt) > 0.f ? accx[v] : 0.f;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ga), or_, vgo, (rb0 + (v & 3) + 8 * (v >> 2)) * go_pitch4, 0);
                cb += ga;
                cg = fmaf(ga, fmaf(zp[v], pi, npm), cg);
            }
        }
    }
    // ---- this workgroup's partial dW block (zeros if it had no tile: dw_reduce sums every block)
    float* pout = partial + (size_t)blockIdx.x * N * Kp;
    {
        const int vs = (4 * half * Kp + kx) * 4, sbase = (blockIdx.x * N + wm * 32) * Kp * 4;       // (< 2^31: the slab is <= 36 MB)
#pragma unroll
        for (int it = 0; it < NIT; ++it)
#pragma unroll
            for (int v = 0; v < 16; ++v)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(accw[it][v]), sr_, vs, sbase + (it * 64 + (v & 3) + 8 * (v >> 2)) * Kp * 4, 0);
    }
    __syncthreads();                                      // the tile loop's last LDS reads are done: As / Ws are free
    if (coords) {
        float* red = smem;                                // [4 wavefronts = row quarters][N][3]
#pragma unroll
        for (int it = 0; it < NIT; ++it)
#pragma unroll
            for (int dd = 0; dd < 3; ++dd) red[(wave * N + it * 64 + lane) * 3 + dd] = wx[it][dd];
        __syncthreads();
        for (int i = tid; i < N * 3; i += 256)
            pout[(size_t)(i / 3) * Kp + x.feat_c + i % 3] = red[i] + red[N * 3 + i] + red[2 * N * 3 + i] + red[3 * N * 3 + i];
        __syncthreads();
    }
    if (!L1) {
        const int rep = blockIdx.x % GAD_STAT_REPLICAS;
        const float c0[1] = {cb}, c1[1] = {cg};
        block_column_atomics<2, 2, 1>(smem, c0, c1, lane, wm, wn, k0, e.k_valid, e.dbeta + (size_t)rep * e.stat_stride,
                                      e.dgamma + (size_t)rep * e.stat_stride);
    }
}

// workgroups per k block of a fused wide launch = partial dW blocks it writes (bwd_wideable checks the workspace against it and hands it on)
static int bwd_wide_splits(const gad_gemm_dx_args& ax) {
    const long long per = (long long)ax.n_out[0] * ax.Kp;
    long long g = (long long)g_opt.bwd_wide_slab * 1000000ll / per;
    const int tiles = gad_cdiv(ax.n_rows, 64);
    const int kb = ax.k_valid / 64;
    if (g * kb > 1024) g = 1024 / kb;                    // (no more workgroups than fit the chip at once)
    if (g > tiles) g = tiles;
    if (g < 16) g = 16 < tiles ? 16 : tiles;
    return (int)g;
}

// ------------------------------------------------------------------------------------------------
// dX and dW of one layer in one call.  The SA1 layers the two streaming kernels cover take the fused kernel
// (gemm_bwd_stream_kernel); everything else runs gad_gemm_dw then gad_gemm_dx on the same stream.
// ------------------------------------------------------------------------------------------------
// the fused wide backward covers what gemm_dx_wide + gemm_dw_wide cover together: one group, BatchNorm + ReLU on both
// sides (premasked gradients), N in {128, 256, 512}, K a multiple of 64; the gathered first layers with their scatter epilogue
static bool bwd_wideable(const gad_gemm_dx_args& ax, const gad_gemm_dw_args& aw, bool vec, int& splits) {
    const gad_gemm_fwd_args& in = aw.in;
    if (g_opt.deterministic || !g_opt.bwd_wide || !vec || ax.n_groups != 1 || in.n_groups != 1) return false;
    if (ax.dz_off[0] != 0 || ax.w_off[0] != 0 || ax.gout_off[0] != 0 || in.zin_off[0] != 0 || aw.dz_off[0] != 0) return false;
    const int N = ax.n_out[0];
    if (N != 128 && N != 256 && N != 512) return false;
    if (ax.n_rows < 2048 || (g_opt.bwd_wide == 2 && ax.n_rows < 16384) || ax.n_rows != in.n_rows || ax.n_rows_dev != in.n_rows_dev) return false;
    if (in.n_out[0] != N || in.Kp != ax.Kp || in.ones_col >= 0 || !aw.partial || !aw.gacc || !ax.W) return false;
    if (ax.k_valid % 64 != 0 || ax.k_valid < 64) return false;
    if ((long long)(splits = bwd_wide_splits(ax)) * N * ax.Kp > aw.partial_elems) return false;   // (workspace of another route)
    const gad_dz_src& d = ax.dz;
    if (!d.z || d.z_pitch % 4 != 0 || !d.relu || !d.premasked || !(d.coefP && d.coefQ && d.coefS)) return false;
    if (d.gmode == 0 ? (d.g_pitch % 4 != 0 || !d.G) : (d.c % 4 != 0 || !d.argmax || !d.dout || !d.row_grp)) return false;
    // both descriptions are of the same layer
    if (d.z != aw.dz.z || d.gmode != aw.dz.gmode || d.G != aw.dz.G || d.dout != aw.dz.dout || d.argmax != aw.dz.argmax ||
        d.row_w != aw.dz.row_w || d.coefP != aw.dz.coefP) return false;
    if (ax.epilogue == 1) {                              // gathered first layer: scatter into the points' feature gradients
        if (in.mode != 1 || d.gmode != 0 || !ax.dfeat || ax.daction || !ax.row_pt || ax.prev_dbeta || in.act_c != 0) return false;
        if (in.feat_c % 64 != 0 || in.feat_c > 512 || ax.k_valid != in.feat_c || ax.feat_c != in.feat_c) return false;
        return in.Kp == ((in.feat_c + 3 + 7) & ~7) && in.row_pt == ax.row_pt;
    }
    if (in.mode != 0 || !ax.prev_dbeta || !ax.store_masked || !ax.gout) return false;
    if (!(ax.zprev && ax.prev_scale && ax.prev_shift && ax.prev_mean && ax.prev_istd && ax.prev_dgamma)) return false;
    if (in.Kp % 64 != 0 || in.Kp > 512 || in.c_in != in.Kp || ax.k_valid != in.Kp || !in.scale || !in.shift || !in.relu || in.extra) return false;
    return in.zin == ax.zprev && in.scale == ax.prev_scale && in.shift == ax.prev_shift && in.zin_pitch == ax.zprev_pitch;
}

static bool bwd_streamable(const gad_gemm_dx_args* ax, const gad_gemm_dw_args* aw) {
    const gad_gemm_fwd_args& in = aw->in;
    if (g_opt.deterministic || !g_opt.bwd_fused) return false;
    const bool vec = dz_vectorizable(ax->dz, ax->dz_off, ax->n_out, ax->n_groups);
    int k_used = in.mode == 0 ? in.c_in + (in.extra ? 1 : 0) : in.feat_c + 3 + in.act_c;
    bool fused = dx_streamable(*ax, vec) && dw_streamable(*aw, k_used);
    // the two descriptions must be of the same layer: same dZ source, and dW's input = the layer dX feeds
    return fused && ax->dz.z == aw->dz.z && ax->dz.gmode == aw->dz.gmode && ax->dz.G == aw->dz.G && ax->dz.dout == aw->dz.dout &&
           ax->dz.argmax == aw->dz.argmax && ax->dz.row_w == aw->dz.row_w && ax->n_rows == in.n_rows && ax->n_rows_dev == in.n_rows_dev &&
           ax->n_out[0] == in.n_out[0] && in.zin == ax->zprev && in.scale == ax->prev_scale && in.shift == ax->prev_shift &&
           in.zin_pitch == 64 && ax->gout && ax->prev_dgamma;
}

// what gad_gemm_bwd does with a (dx, dw) pair, decided here alone: a deferred gad_gemm_dw_reduce made under the same options sums
// exactly the partial dW blocks the kernel wrote.  splits: those blocks; Kp, k_used: of the reduce
struct BwdRoute { enum { UNFUSED, WIDE, STREAM } kind; int splits, Kp, k_used; };

static BwdRoute bwd_route(const gad_gemm_dx_args& ax, const gad_gemm_dw_args& aw) {
    const int wgs = g_opt.bwd_stream_wgs, Kp = aw.in.Kp;
    int wide = 0;                                                      // (the fused wide launch's blocks: bwd_wideable sets it)
    // (the SA1 shapes: the streaming kernel has precedence; splits = the partial dW blocks the kernel writes, see its header)
    if (bwd_streamable(&ax, &aw)) return {BwdRoute::STREAM, ax.n_out[0] == 64 ? 2 * wgs : wgs, 64, 64};
    if (bwd_wideable(ax, aw, dz_vectorizable(ax.dz, ax.dz_off, ax.n_out, ax.n_groups), wide)) return {BwdRoute::WIDE, wide, Kp, aw.in.mode == 1 ? aw.in.feat_c + 3 : Kp};
    return {BwdRoute::UNFUSED, 0, 0, 0};
}

static int bwd_reduce(const BwdRoute& r, const gad_gemm_dx_args* ax, const gad_gemm_dw_args* aw, void* stream) {
    Groups gr = make_groups(1, aw->dz_off, aw->in.w_off, aw->in.zin_off, aw->in.n_out);
    return dw_reduce_launch(aw->partial, gr, aw->in.n_out[0], aw->in.n_rows_dev, ax->n_rows, r.splits, r.Kp, r.k_used, aw->gacc, 1, (hipStream_t)stream);
}

// the reduce launch of a fused backward call whose aw->row_splits was GAD_DW_REDUCE_LATER (include/gaddpg.h): sums the partial
// dW blocks that call left in aw->partial into the arena.  A layer gad_gemm_bwd does not fuse has reduced already: no-op.
extern "C" int gad_gemm_dw_reduce(const gad_gemm_dx_args* ax, const gad_gemm_dw_args* aw, void* stream) {
    GAD_REQUIRE(ax && aw, GAD_ERR_NULL, "gemm_dw_reduce: null pointer");
    if (ax->n_rows <= 0) return GAD_OK;
    const BwdRoute r = bwd_route(*ax, *aw);
    return r.kind == BwdRoute::UNFUSED ? GAD_OK : bwd_reduce(r, ax, aw, stream);
}

extern "C" int gad_gemm_bwd(const gad_gemm_dx_args* ax, const gad_gemm_dw_args* aw, void* stream) {
    GAD_REQUIRE(ax && aw, GAD_ERR_NULL, "gemm_bwd: null pointer");
    const gad_gemm_fwd_args& in = aw->in;
    const bool later = aw->row_splits == GAD_DW_REDUCE_LATER;          // the caller launches gad_gemm_dw_reduce itself
    const BwdRoute r = bwd_route(*ax, *aw);
    if (r.kind == BwdRoute::UNFUSED) {
        gad_gemm_dw_args aw2 = *aw;
        if (later) aw2.row_splits = 0;
        if (int e = gad_gemm_dw(&aw2, stream)) return e;
        return gad_gemm_dx(ax, stream);
    }
    unsigned long long* ts = gad_take_timing_slot(stream);
    (void)gad_take_grid_rows();
    hipStream_t st = (hipStream_t)stream;
    if (r.kind == BwdRoute::WIDE) {
        if (ax->n_rows <= 0) return GAD_OK;
        const int N = ax->n_out[0], splits = r.splits;
        GAD_REQUIRE((long long)splits * N * in.Kp <= aw->partial_elems, GAD_ERR_SHAPE, "gemm_bwd(wide): partial workspace too small (%lld floats needed)",
                    (long long)splits * N * in.Kp);
        DzSrc d = make_dzsrc(ax->dz);
        XSrc x = make_xsrc(in);
        DxEpi e = make_dxepi(*ax);                                    // stores masked; the feature scatter only (bwd_wideable: no daction)
        e.store_masked = 1;
        e.daction = nullptr; e.act_c = 0; e.gps = 1;
        const dim3 grid(splits, ax->k_valid / 64);
#define LAUNCH_BWW(NIT, GM, L1) hipLaunchKernelGGL((gemm_bwd_wide_kernel<NIT, GM, L1>), grid, dim3(256), 0, st, d, x, ax->n_rows_dev, ax->n_rows, ax->W, ax->Kp, e, aw->partial, ts)
        const bool l1 = ax->epilogue == 1, pooled = ax->dz.gmode != 0;
        if (N == 128) { if (l1) LAUNCH_BWW(2, 0, 1); else if (pooled) LAUNCH_BWW(2, 1, 0); else LAUNCH_BWW(2, 0, 0); }
        else if (N == 256) { if (l1) LAUNCH_BWW(4, 0, 1); else if (pooled) LAUNCH_BWW(4, 1, 0); else LAUNCH_BWW(4, 0, 0); }
        else { if (l1) LAUNCH_BWW(8, 0, 1); else if (pooled) LAUNCH_BWW(8, 1, 0); else LAUNCH_BWW(8, 0, 0); }
#undef LAUNCH_BWW
        GAD_CHECK_LAUNCH("gemm_bwd(wide)");
        return later ? GAD_OK : bwd_reduce(r, ax, aw, stream);
    }
    GAD_REQUIRE(aw->gacc && ax->W, GAD_ERR_NULL, "gemm_bwd: null pointer");
    if (ax->n_rows <= 0) return GAD_OK;
    DzSrc d = make_dzsrc(ax->dz);
    DxEpi e = make_dxepi(*ax);                                        // stores masked, scatters nothing
    e.mode = 0; e.store_masked = 1;
    e.dfeat = nullptr; e.feat_c = 0; e.row_pt = nullptr; e.row_grp = nullptr; e.daction = nullptr; e.act_c = 0; e.gps = 1;
    const int rows = ax->n_rows, wgs = g_opt.bwd_stream_wgs;
    GAD_REQUIRE((long long)r.splits * in.n_out[0] * 64 <= aw->partial_elems, GAD_ERR_SHAPE, "gemm_bwd: partial workspace too small");
    // (a pooled source with 64 outputs -- no layer of the step: SA1 pools its 128-output layer -- keeps the FP32-MFMA kernel: the
    // fused split instantiation <8, 1, true> left channels 0 .. 31 of dW ~1e-2 off the float64 reference on an MI355X while its dX was
    // exact, tests/test_gpu_gemm_f64_wide.py table E; the cause is not found)
    if (split_on(GAD_SPLIT_BWD_STREAM) && ax->W_split_t && ax->W_split_t_pitch == ax->n_out[0] && ax->W_split_t_plane >= 64 * ax->n_out[0] &&
        !(ax->dz.gmode != 0 && ax->n_out[0] == 64)) {
#define LAUNCH_BWSS(NJ, GM) hipLaunchKernelGGL((gemm_bwd_stream_split_kernel<NJ, GM, true>), dim3(wgs), dim3(512), 0, st, d, ax->n_rows_dev, rows, \
                                                ax->W_split_t, ax->W_split_t_plane, e, aw->partial, ts)
        if (ax->n_out[0] == 128) { if (ax->dz.gmode == 0) LAUNCH_BWSS(16, 0); else LAUNCH_BWSS(16, 1); }
        else LAUNCH_BWSS(8, 0);
#undef LAUNCH_BWSS
        GAD_CHECK_LAUNCH("gemm_bwd(stream split)");
        return later ? GAD_OK : bwd_reduce(r, ax, aw, stream);
    }
#define LAUNCH_BWS(NJ, GM) hipLaunchKernelGGL((gemm_bwd_stream_kernel<NJ, GM>), dim3(wgs), dim3(512), 0, st, d, ax->n_rows_dev, rows, ax->W, e, aw->partial, ts)
    if (ax->n_out[0] == 128) { if (ax->dz.gmode == 0) LAUNCH_BWS(16, 0); else LAUNCH_BWS(16, 1); }
    else { if (ax->dz.gmode == 0) LAUNCH_BWS(8, 0); else LAUNCH_BWS(8, 1); }
#undef LAUNCH_BWS
    GAD_CHECK_LAUNCH("gemm_bwd(stream)");
    return later ? GAD_OK : bwd_reduce(r, ax, aw, stream);
}
